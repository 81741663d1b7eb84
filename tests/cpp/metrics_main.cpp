// Exercises the C++20 facade's image error (path_tracer_amd/include/pt/path_tracer.hpp: pt::image_error, pt::image_error_params,
// pt::image_error_result): reads from <in.bin> two frames a and ref (float32 [h][w][3] each); runs the stage inside the rectangle
// <x0> <y0> <x1> <y1> (four zeros: the whole frame) once with the error plane and once more under no_lds without it, and writes to
// <out.bin>: the first call's PtImageErrorResult, its plane (float32 [h][w]), the second call's PtImageErrorResult.  It prints the first
// call's derived figures.  Every buffer is device memory the program allocates (HIP runtime).
//
//   metrics_main <w> <h> <x0> <y0> <x1> <y1> <in.bin> <out.bin>
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "pt/path_tracer.hpp"

using namespace pt;

int main(int argc, char** argv) {
  if (argc < 9) { std::fprintf(stderr, "usage: metrics_main <w> <h> <x0> <y0> <x1> <y1> <in.bin> <out.bin>\n"); return 2; }
  const int w = std::atoi(argv[1]), h = std::atoi(argv[2]);
  image_error_params ip;
  for (int i = 0; i < 4; i++) ip.rect[i] = std::atoi(argv[3 + i]);
  const size_t n1 = (size_t)w * h, n3 = n1 * 3;
  std::vector<float> host(2 * n3);
  {
    std::ifstream in(argv[7], std::ios::binary);
    in.read(reinterpret_cast<char*>(host.data()), (std::streamsize)(2 * n3 * sizeof(float)));
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[7]); return 1; }
  }
  float* frames = nullptr;
  float* plane = nullptr;
  PtImageErrorResult* result = nullptr;
  void* scratch = nullptr;
  if (hipMalloc((void**)&frames, 2 * n3 * sizeof(float)) != hipSuccess || hipMalloc((void**)&plane, n1 * sizeof(float)) != hipSuccess ||
      hipMalloc((void**)&result, sizeof(PtImageErrorResult)) != hipSuccess || hipMalloc(&scratch, image_error_scratch_bytes()) != hipSuccess) {
    std::fprintf(stderr, "hipMalloc failed\n");
    return 1;
  }
  int rc = 0;
  try {
    if (hipMemcpy(frames, host.data(), 2 * n3 * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("hipMemcpy failed");
    std::ofstream file(argv[8], std::ios::binary);
    std::vector<char> back(std::max(n1 * sizeof(float), sizeof(PtImageErrorResult)));
    auto get = [&](const void* device, size_t size) { // (hipMemcpy waits for the null stream's work)
      if (hipMemcpy(back.data(), device, size, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("hipMemcpy failed");
      file.write(back.data(), (std::streamsize)size);
    };
    image_error(w, h, frames, frames + n3, result, scratch, plane, ip);
    get(result, sizeof(PtImageErrorResult));
    image_error_result r;
    std::memcpy(static_cast<PtImageErrorResult*>(&r), back.data(), sizeof(PtImageErrorResult));
    get(plane, n1 * sizeof(float));
    ip.no_lds = true;
    image_error(w, h, frames, frames + n3, result, scratch, nullptr, ip);
    get(result, sizeof(PtImageErrorResult));
    std::printf("%dx%d: MSE %.17g MAE %.17g relMSE %.17g PSNR %.17g pixels %llu skipped %llu\n", w, h, r.mse(), r.mae(), r.rel_mse(), r.psnr(1.0),
                (unsigned long long)r.pixels, (unsigned long long)r.skipped);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    rc = 1;
  }
  (void)hipFree(frames); (void)hipFree(plane); (void)hipFree(result); (void)hipFree(scratch);
  return rc;
}
