// Exercises the C++20 facade's denoiser (path_tracer_amd/include/pt/path_tracer.hpp: pt::denoise, pt::denoise_params) on the Cornell-style
// scene of facade_main.cpp: the frame at <samples> spp, the guides of pt::render_aov at <aov samples>, the filter with the header's
// defaults, then the filter again in place (out = color) with three iterations and no demodulation.  Writes both filtered frames
// (float32 [h][w][3] each) to one file.  Every buffer is device memory the program allocates (HIP runtime).
//
//   denoise_main <w> <h> <samples> <aov samples> <out.bin>
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
  if (argc < 6) { std::fprintf(stderr, "usage: denoise_main <w> <h> <samples> <aov samples> <out.bin>\n"); return 2; }
  const int w = std::atoi(argv[1]), h = std::atoi(argv[2]), samples = std::atoi(argv[3]), aov_samples = std::atoi(argv[4]);
  const std::string out = argv[5];
  const int64_t n1 = (int64_t)w * h, n3 = 3 * n1, ns = denoise_scratch_floats(w, h);
  if (ns < 11 * n1) { std::fprintf(stderr, "denoise_scratch_floats: %lld\n", (long long)ns); return 1; }
  // one device allocation: the frame, albedo, normal, the filtered frame (4 x n3), depth (n1), then the scratch, 16-byte aligned
  const size_t head = (size_t)((4 * n3 + n1 + 3) / 4 * 4);
  float* dev = nullptr;
  if (hipMalloc((void**)&dev, (head + (size_t)ns) * sizeof(float)) != hipSuccess) { std::fprintf(stderr, "hipMalloc failed\n"); return 1; }
  int rc = 0;
  try {
    float *fb = dev, *albedo = dev + n3, *normal = dev + 2 * n3, *filtered = dev + 3 * n3, *depth = dev + 4 * n3, *scratch = dev + head;
    const camera cam(point{278, 278, -800}, point{278, 278, 0}, vec{0, 1, 0}, 40, (float)w / (float)h, 0, 800, 0, 1);
    device_scene scene(cornell());
    const PtRenderParams p{w, h, samples, 50, 0, 1, 0, 0};
    check(pt_render(scene.s, &cam.c, &p, fb, nullptr), "pt_render");
    aov_buffers b;
    b.albedo = albedo; b.normal = normal; b.depth = depth;
    render_aov(w, h, aov_samples, b, scene, cam);
    denoise(w, h, fb, albedo, normal, depth, filtered, scratch);
    denoise_params plain;
    plain.iterations = 3; plain.demodulate = false;
    denoise(w, h, fb, albedo, normal, depth, fb, scratch, plain); // in place
    if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("hipDeviceSynchronize failed");
    std::vector<float> host((size_t)(2 * n3));
    if (hipMemcpy(host.data(), filtered, (size_t)n3 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("hipMemcpy failed");
    if (hipMemcpy(host.data() + n3, fb, (size_t)n3 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("hipMemcpy failed");
    std::ofstream f(out, std::ios::binary);
    f.write(reinterpret_cast<const char*>(host.data()), (std::streamsize)(host.size() * sizeof(float)));
    std::printf("%dx%d, %d spp, guides at %d: denoised (defaults), denoised in place (3 iterations, plain)\n", w, h, samples, aov_samples);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    rc = 1;
  }
  (void)hipFree(dev);
  return rc;
}
