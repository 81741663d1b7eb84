// Exercises the C++20 facade's adaptive sampling (path_tracer_amd/include/pt/path_tracer.hpp: pt::accumulator constructed with
// pt::adaptive) on the Cornell-style scene of facade_main.cpp: render.render_adaptive's loop — a window of min_spp samples of every pixel,
// then windows of `step` samples of the pixels pt_adaptive_select keeps active (dilated), unmasked when every pixel is — optionally
// checkpointed after the first window and resumed in a NEW accumulator over a new device scene — or (--plain-checkpoint) that first
// window rendered by a PLAIN accumulator, saved, and loaded into the adaptive one.  Writes the resolved frame buffer
// (float32 [h][w][3]) and the per-pixel counts (int32 [h][w]).  The mask is a device buffer the program allocates (HIP runtime).
//
//   adaptive_main <w> <h> <out.f32> <counts.i32> <threshold> <min_spp> <max_spp> <step> [--checkpoint | --plain-checkpoint <state file>]
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
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
  if (argc < 9) { std::fprintf(stderr, "usage: see the file header\n"); return 2; }
  const int w = std::atoi(argv[1]), h = std::atoi(argv[2]);
  const std::string out = argv[3], counts_out = argv[4];
  const float threshold = (float)std::atof(argv[5]);
  const int min_spp = std::atoi(argv[6]), max_spp = std::atoi(argv[7]), step = std::atoi(argv[8]);
  std::string checkpoint;
  bool from_plain = false;
  for (int i = 9; i < argc; i++) {
    if (std::strcmp(argv[i], "--checkpoint") == 0 && i + 1 < argc) checkpoint = argv[++i];
    else if (std::strcmp(argv[i], "--plain-checkpoint") == 0 && i + 1 < argc) { checkpoint = argv[++i]; from_plain = true; }
  }
  uint8_t* mask = nullptr;
  if (hipMalloc((void**)&mask, (size_t)w * h) != hipSuccess) { std::fprintf(stderr, "hipMalloc failed\n"); return 1; }
  int windows = 1;
  try {
    const std::vector<hittable_t> hittables = cornell();
    const camera cam(point{278, 278, -800}, point{278, 278, 0}, vec{0, 1, 0}, 40, (float)w / (float)h, 0, 800, 0, 1);
    auto scene = std::make_unique<device_scene>(hittables);
    std::unique_ptr<accumulator> acc;
    if (from_plain) { // the first window in a plain accumulator, continued adaptively from its checkpoint
      accumulator plain(*scene, cam, w, h);
      plain.add(min_spp);
      plain.save(checkpoint);
      acc = std::make_unique<accumulator>(adaptive, *scene, cam, w, h);
      acc->load(checkpoint);
    } else {
      acc = std::make_unique<accumulator>(adaptive, *scene, cam, w, h);
      acc->add(min_spp);
    }
    if (!checkpoint.empty() && !from_plain) { // checkpoint, drop everything, resume in a new accumulator over a new device scene
      acc->save(checkpoint);
      acc.reset();
      scene = std::make_unique<device_scene>(hittables);
      acc = std::make_unique<accumulator>(adaptive, *scene, cam, w, h);
      acc->load(checkpoint);
    }
    for (;;) {
      const int64_t n_active = acc->select(threshold, min_spp, max_spp, true, mask);
      if (n_active == 0) break;
      acc->add_masked(step, n_active == (int64_t)w * h ? nullptr : mask);
      windows++;
    }
    frame_buffer fb;
    acc->resolve(fb);
    const std::vector<int32_t> n = acc->counts();
    std::ofstream f(out, std::ios::binary);
    f.write(reinterpret_cast<const char*>(fb.data()), (std::streamsize)(fb.size() * sizeof(color)));
    std::ofstream c(counts_out, std::ios::binary);
    c.write(reinterpret_cast<const char*>(n.data()), (std::streamsize)(n.size() * sizeof(int32_t)));
    double mean = 0;
    for (int32_t v : n) mean += v;
    std::printf("%dx%d, adaptive %d..%d spp in %d windows, mean %.2f spp\n", w, h, min_spp, max_spp, windows, mean / (double)n.size());
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    (void)hipFree(mask);
    return 1;
  }
  (void)hipFree(mask);
  return 0;
}
