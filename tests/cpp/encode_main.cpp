// Exercises the C++20 facade's encode stage (path_tracer_amd/include/pt/path_tracer.hpp: pt::encode, pt::encode_params,
// pt::display_encode): reads from <in.bin> one frame (float32 [h][w][3]) and writes to <out.bin> four images of [h][w][3] bytes: the sRGB
// codes; the dithered codes at phase (3, 5); the fused call with the ACES curve at <ev> stops, dithered at phase (3, 5); the reference
// transfer.  With <out.png> the first image is also written as a PNG tagged sRGB (pt/image_io.hpp).  Every buffer is device memory the
// program allocates (HIP runtime).
//
//   encode_main <w> <h> <ev> <in.bin> <out.bin> [<out.png>]
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <stdexcept>
#include <vector>

#include "pt/image_io.hpp"
#include "pt/path_tracer.hpp"

using namespace pt;

int main(int argc, char** argv) {
  if (argc < 6) { std::fprintf(stderr, "usage: encode_main <w> <h> <ev> <in.bin> <out.bin> [<out.png>]\n"); return 2; }
  const int w = std::atoi(argv[1]), h = std::atoi(argv[2]);
  const float ev = (float)std::atof(argv[3]);
  const size_t n3 = (size_t)w * h * 3;
  std::vector<float> host(n3);
  {
    std::ifstream in(argv[4], std::ios::binary);
    in.read(reinterpret_cast<char*>(host.data()), (std::streamsize)(n3 * sizeof(float)));
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[4]); return 1; }
  }
  float* frame = nullptr;
  uint8_t* rgb8 = nullptr;
  if (hipMalloc((void**)&frame, n3 * sizeof(float)) != hipSuccess || hipMalloc((void**)&rgb8, n3) != hipSuccess) {
    std::fprintf(stderr, "hipMalloc failed\n");
    return 1;
  }
  int rc = 0;
  try {
    if (hipMemcpy(frame, host.data(), n3 * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("hipMemcpy failed");
    std::ofstream file(argv[5], std::ios::binary);
    std::vector<uint8_t> back(n3);
    auto get = [&]() { // (hipMemcpy waits for the null stream's work)
      if (hipMemcpy(back.data(), rgb8, n3, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("hipMemcpy failed");
      file.write(reinterpret_cast<const char*>(back.data()), (std::streamsize)n3);
    };
    encode(w, h, frame, rgb8);
    get();
    if (argc > 6 && !image_io::write_png(argv[6], back.data(), (size_t)w, (size_t)h, true)) throw std::runtime_error("cannot write the PNG");
    encode_params ep;
    ep.dither = true; ep.phase_x = 3; ep.phase_y = 5;
    encode(w, h, frame, rgb8, ep);
    get();
    display_params dp;
    dp.tone = PT_TONE_ACES; dp.ev_bias = ev;
    display_encode(w, h, frame, rgb8, dp, ep);
    get();
    encode_params ref;
    ref.transfer = PT_TRANSFER_REFERENCE;
    encode(w, h, frame, rgb8, ref);
    get();
    std::printf("%dx%d: four images of %zu bytes\n", w, h, n3);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    rc = 1;
  }
  (void)hipFree(frame); (void)hipFree(rgb8);
  return rc;
}
