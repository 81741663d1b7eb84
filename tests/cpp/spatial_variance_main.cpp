// Exercises the C++20 facade's spatial variance estimate (path_tracer_amd/include/pt/path_tracer.hpp: pt::spatial_variance,
// pt::spatial_variance_params, pt::spatial_variance_guides): reads from <in.bin> a frame, its albedo and normal planes and a variance plane
// (float32 [h][w][3] each), then its depth plane (float32 [h][w]) and its id plane (int32 [h][w]); runs the stage with <radius> and
// <min_pairs> once without a variance plane and with counts, and once more in fill mode with variance_out aliasing variance_in, and writes
// to <out.bin>: the first call's plane, its two counts (uint32), the second call's plane and its two counts.  Every buffer is device memory
// the program allocates (HIP runtime).
//
//   spatial_variance_main <w> <h> <radius> <min_pairs> <in.bin> <out.bin>
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "pt/path_tracer.hpp"

using namespace pt;

int main(int argc, char** argv) {
  if (argc < 7) { std::fprintf(stderr, "usage: spatial_variance_main <w> <h> <radius> <min_pairs> <in.bin> <out.bin>\n"); return 2; }
  const int w = std::atoi(argv[1]), h = std::atoi(argv[2]);
  spatial_variance_params sp;
  sp.radius = std::atoi(argv[3]);
  sp.min_pairs = std::atoi(argv[4]);
  const size_t n1 = (size_t)w * h, n3 = n1 * 3;
  const size_t in_floats = 4 * n3 + 2 * n1; // color, albedo, normal, variance, depth, id
  std::vector<float> host(in_floats);
  {
    std::ifstream in(argv[5], std::ios::binary);
    in.read(reinterpret_cast<char*>(host.data()), (std::streamsize)(in_floats * sizeof(float)));
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[5]); return 1; }
  }
  // one device allocation: the inputs as they lie in the file, the output plane (n3 floats) and the two counts
  float* dev = nullptr;
  if (hipMalloc((void**)&dev, (in_floats + n3) * sizeof(float) + 2 * sizeof(uint32_t)) != hipSuccess) { std::fprintf(stderr, "hipMalloc failed\n"); return 1; }
  int rc = 0;
  try {
    float *color = dev, *albedo = dev + n3, *normal = dev + 2 * n3, *variance = dev + 3 * n3, *depth = dev + 4 * n3;
    const int32_t* id = reinterpret_cast<const int32_t*>(dev + 4 * n3 + n1);
    float* out = dev + in_floats;
    uint32_t* counts = reinterpret_cast<uint32_t*>(dev + in_floats + n3); // (8-byte aligned: an even number of floats lies before it)
    static_assert(sizeof(float) == 4, "the layout above counts in 4-byte words");
    if (((in_floats + n3) & 1) != 0) throw std::runtime_error("w x h must be even for this program's layout");
    auto sync = [] { if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("hipDeviceSynchronize failed"); };
    if (hipMemcpy(dev, host.data(), in_floats * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("hipMemcpy failed");
    std::ofstream file(argv[6], std::ios::binary);
    std::vector<float> back(n3);
    auto put = [&](const void* device, size_t size) {
      if (hipMemcpy(back.data(), device, size, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("hipMemcpy failed");
      file.write(reinterpret_cast<const char*>(back.data()), (std::streamsize)size);
    };
    const spatial_variance_guides g{albedo, normal, depth, id};
    spatial_variance(w, h, color, g, nullptr, out, counts, sp);
    sync();
    put(out, n3 * sizeof(float));
    put(counts, 2 * sizeof(uint32_t));
    spatial_variance(w, h, color, g, variance, variance, counts, sp); // fill mode, in place
    sync();
    put(variance, n3 * sizeof(float));
    put(counts, 2 * sizeof(uint32_t));
    std::printf("%dx%d, radius %d, min_pairs %d: spatial variance estimate\n", w, h, sp.radius, sp.min_pairs);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    rc = 1;
  }
  (void)hipFree(dev);
  return rc;
}
