// Exercises the C++20 facade's first-hit feature buffers (path_tracer_amd/include/pt/path_tracer.hpp: pt::aov_buffers, pt::render_aov)
// on the Cornell-style scene of facade_main.cpp: all six planes of one pass over a device_scene, and — the second overload — the
// albedo plane again from the list of hittables.  Writes the planes to one file, in PtAovBuffers' order: albedo, normal, direct
// (float32 [h][w][3]), depth, coverage (float32 [h][w]), id (int32 [h][w]), then the second albedo.  The planes are device buffers
// the program allocates (HIP runtime).
//
//   aov_main <w> <h> <samples> <out.bin>
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
  if (argc < 5) { std::fprintf(stderr, "usage: aov_main <w> <h> <samples> <out.bin>\n"); return 2; }
  const int w = std::atoi(argv[1]), h = std::atoi(argv[2]), samples = std::atoi(argv[3]);
  const std::string out = argv[4];
  const int64_t n1 = aov_plane_elems(w, h, 1), n3 = aov_plane_elems(w, h, 3);
  if (n1 != (int64_t)w * h || n3 != 3 * n1) { std::fprintf(stderr, "aov_plane_elems: %lld, %lld\n", (long long)n1, (long long)n3); return 1; }
  // one device allocation, cut into the planes: 3 x n3 + 3 x n1 elements, then the second albedo
  const size_t words = (size_t)(4 * n3 + 3 * n1);
  float* dev = nullptr;
  if (hipMalloc((void**)&dev, words * sizeof(float)) != hipSuccess) { std::fprintf(stderr, "hipMalloc failed\n"); return 1; }
  int rc = 0;
  try {
    const std::vector<hittable_t> hittables = cornell();
    const camera cam(point{278, 278, -800}, point{278, 278, 0}, vec{0, 1, 0}, 40, (float)w / (float)h, 0, 800, 0, 1);
    aov_buffers b;
    b.albedo = dev; b.normal = dev + n3; b.direct = dev + 2 * n3;
    b.depth = dev + 3 * n3; b.coverage = dev + 3 * n3 + n1; b.id = reinterpret_cast<int32_t*>(dev + 3 * n3 + 2 * n1);
    {
      device_scene scene(hittables);
      render_aov(w, h, samples, b, scene, cam);
      if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("hipDeviceSynchronize failed");
    }
    aov_buffers again;
    again.albedo = dev + 3 * n3 + 3 * n1;
    render_aov(w, h, samples, again, hittables, cam);
    std::vector<float> host(words);
    if (hipMemcpy(host.data(), dev, words * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("hipMemcpy failed");
    std::ofstream f(out, std::ios::binary);
    f.write(reinterpret_cast<const char*>(host.data()), (std::streamsize)(words * sizeof(float)));
    std::printf("%dx%d, %d samples: 6 planes + albedo from the hittables\n", w, h, samples);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    rc = 1;
  }
  (void)hipFree(dev);
  return rc;
}
