// Exercises the C++20 facade's variance-guided denoiser (path_tracer_amd/include/pt/path_tracer.hpp: pt::accumulator::variance,
// pt::variance_denoise, pt::variance_denoise_params) on the Cornell-style scene of facade_main.cpp: an adaptive accumulator after two
// windows of <window> samples, its resolved frame and variance estimate, the guides of pt::render_aov at <aov samples>, the filter with
// the header's defaults (and the residual variance), then the filter again in place (out = color, variance_out = variance) with three
// iterations and no demodulation.  Writes the filtered frame, its residual variance, the in-place frame and the in-place variance
// (float32 [h][w][3] each) to one file.  Every buffer is device memory the program allocates (HIP runtime).
//
//   variance_denoise_main <w> <h> <window> <aov samples> <out.bin>
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "pt/path_tracer.hpp"

using namespace pt;

static std::vector<hittable_t> cornell() {
  material_t white = lambertian_material(color{0.73f, 0.73f, 0.73f});
  material_t red = lambertian_material(color{0.65f, 0.05f, 0.05f});
  material_t green = lambertian_material(color{0.12f, 0.45f, 0.15f});
  material_t light = lightsource_material(color{15.0f, 15.0f, 15.0f});
  std::vector<hittable_t> h;
  h.emplace_back(box(point{555, 0, 0}, point{556, 555, 555}, green));
  h.emplace_back(box(point{-1, 0, 0}, point{0, 555, 555}, red));
  h.emplace_back(box(point{213, 554, 227}, point{343, 554.5f, 332}, light));
  h.emplace_back(box(point{0, -1, 0}, point{555, 0, 555}, white));
  h.emplace_back(box(point{0, 555, 0}, point{555, 556, 555}, white));
  h.emplace_back(xy_rect(0, 555, 0, 555, 555, white));
  h.emplace_back(box(point{130, 0, 65}, point{295, 165, 230}, white));
  h.emplace_back(box(point{265, 0, 295}, point{430, 330, 460}, white));
  return h;
}

int main(int argc, char** argv) {
  if (argc < 6) { std::fprintf(stderr, "usage: variance_denoise_main <w> <h> <window> <aov samples> <out.bin>\n"); return 2; }
  const int w = std::atoi(argv[1]), h = std::atoi(argv[2]), window = std::atoi(argv[3]), aov_samples = std::atoi(argv[4]);
  const std::string out = argv[5];
  const int64_t n1 = (int64_t)w * h, n3 = 3 * n1, ns = variance_denoise_scratch_floats(w, h);
  if (ns != 20 * n1) { std::fprintf(stderr, "variance_denoise_scratch_floats: %lld\n", (long long)ns); return 1; }
  // one device allocation: the frame, its variance, albedo, normal, the filtered frame, its variance (6 x n3), depth (n1), then the
  // scratch, 16-byte aligned
  const size_t head = (size_t)((6 * n3 + n1 + 3) / 4 * 4);
  float* dev = nullptr;
  if (hipMalloc((void**)&dev, (head + (size_t)ns) * sizeof(float)) != hipSuccess) { std::fprintf(stderr, "hipMalloc failed\n"); return 1; }
  int rc = 0;
  try {
    float *fb = dev, *var = dev + n3, *albedo = dev + 2 * n3, *normal = dev + 3 * n3, *filtered = dev + 4 * n3, *residual = dev + 5 * n3,
          *depth = dev + 6 * n3, *scratch = dev + head;
    const camera cam(point{278, 278, -800}, point{278, 278, 0}, vec{0, 1, 0}, 40, (float)w / (float)h, 0, 800, 0, 1);
    device_scene scene(cornell());
    accumulator acc(adaptive, scene, cam, w, h);
    acc.add(window);
    acc.add(window);
    check(pt_accum_resolve(acc.handle(), fb, nullptr), "pt_accum_resolve");
    acc.variance(var);
    aov_buffers b;
    b.albedo = albedo; b.normal = normal; b.depth = depth;
    render_aov(w, h, aov_samples, b, scene, cam);
    variance_denoise(w, h, fb, var, albedo, normal, depth, filtered, residual, scratch);
    variance_denoise_params plain;
    plain.iterations = 3; plain.demodulate = false;
    variance_denoise(w, h, fb, var, albedo, normal, depth, fb, var, scratch, plain); // in place, both planes
    if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("hipDeviceSynchronize failed");
    std::vector<float> host((size_t)(4 * n3));
    const float* planes[4] = {filtered, residual, fb, var};
    for (int k = 0; k < 4; k++)
      if (hipMemcpy(host.data() + k * n3, planes[k], (size_t)n3 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("hipMemcpy failed");
    std::ofstream f(out, std::ios::binary);
    f.write(reinterpret_cast<const char*>(host.data()), (std::streamsize)(host.size() * sizeof(float)));
    std::printf("%dx%d, 2 x %d spp, guides at %d: variance-guided filter (defaults), in place (3 iterations, plain)\n", w, h, window, aov_samples);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    rc = 1;
  }
  (void)hipFree(dev);
  return rc;
}
