// Exercises the C++20 facade's firefly stage (path_tracer_amd/include/pt/path_tracer.hpp: pt::firefly, pt::firefly_params): reads a frame
// and its variance plane (float32 [h][w][3] each) from <in.bin>, runs the stage with <rank>, <k> and <repair> (0 / 1) once with separate
// planes and counts, and once more with variance_out aliasing variance and no counts, and writes to <out.bin>: the frame, the variance
// plane, the two counts (uint32), and the second call's frame and variance plane.  Every buffer is device memory the program allocates
// (HIP runtime).
//
//   firefly_main <w> <h> <rank> <k> <repair> <in.bin> <out.bin>
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "pt/path_tracer.hpp"

using namespace pt;

int main(int argc, char** argv) {
  if (argc < 8) { std::fprintf(stderr, "usage: firefly_main <w> <h> <rank> <k> <repair> <in.bin> <out.bin>\n"); return 2; }
  const int w = std::atoi(argv[1]), h = std::atoi(argv[2]);
  firefly_params fp;
  fp.rank = std::atoi(argv[3]);
  fp.k = (float)std::atof(argv[4]);
  fp.repair = std::atoi(argv[5]) != 0;
  const size_t n3 = (size_t)w * h * 3;
  std::vector<float> host(2 * n3);
  {
    std::ifstream in(argv[6], std::ios::binary);
    in.read(reinterpret_cast<char*>(host.data()), (std::streamsize)(2 * n3 * sizeof(float)));
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[6]); return 1; }
  }
  // one device allocation: color, variance, out, variance_out (4 x n3 floats) and the two counts
  float* dev = nullptr;
  if (hipMalloc((void**)&dev, 4 * n3 * sizeof(float) + 2 * sizeof(uint32_t)) != hipSuccess) { std::fprintf(stderr, "hipMalloc failed\n"); return 1; }
  int rc = 0;
  try {
    float *color = dev, *variance = dev + n3, *out = dev + 2 * n3, *variance_out = dev + 3 * n3;
    uint32_t* counts = reinterpret_cast<uint32_t*>(dev + 4 * n3);
    auto sync = [] { if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("hipDeviceSynchronize failed"); };
    if (hipMemcpy(color, host.data(), 2 * n3 * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("hipMemcpy failed");
    std::ofstream file(argv[7], std::ios::binary);
    std::vector<float> back(2 * n3);
    auto put = [&](const void* device, size_t size) {
      if (hipMemcpy(back.data(), device, size, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("hipMemcpy failed");
      file.write(reinterpret_cast<const char*>(back.data()), (std::streamsize)size);
    };
    firefly(w, h, color, variance, out, variance_out, counts, fp);
    sync();
    put(out, 2 * n3 * sizeof(float)); // out and variance_out lie behind one another
    put(counts, 2 * sizeof(uint32_t));
    firefly(w, h, color, variance, out, variance, nullptr, fp); // in place for the variance
    sync();
    put(out, n3 * sizeof(float));
    put(variance, n3 * sizeof(float));
    std::printf("%dx%d, rank %d, k %g, repair %d: firefly stage\n", w, h, fp.rank, (double)fp.k, (int)fp.repair);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    rc = 1;
  }
  (void)hipFree(dev);
  return rc;
}
