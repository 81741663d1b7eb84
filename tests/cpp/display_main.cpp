// Exercises the C++20 facade's display stage (path_tracer_amd/include/pt/path_tracer.hpp: pt::display, pt::display_params,
// pt::display_apply) on the Cornell-style scene of facade_main.cpp: <frames> frames of <spp> samples, frame f looking from
// (278 + f * <move x>, 278, -800), each metered by one pt::display (so the exposure adapts from frame to frame at the given rates) and
// shown through <tone> (0 reference, 1 Reinhard, 2 ACES).  Writes, per frame: the rendered frame and the stage's linear output (float32
// [h][w][3] each), the exposure (one float32), the metering histogram (257 uint32) and the rgb8 image ([h][w][3] bytes, row 0 = top); and
// once at the end the rgb8 image of the last frame through the stateless pt::display_apply at 1 EV.  Every buffer is device memory the
// program allocates (HIP runtime).
//
//   display_main <w> <h> <frames> <spp> <move x> <tone> <adapt up> <adapt down> <out.bin>
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
  if (argc < 10) { std::fprintf(stderr, "usage: display_main <w> <h> <frames> <spp> <move x> <tone> <adapt up> <adapt down> <out.bin>\n"); return 2; }
  const int w = std::atoi(argv[1]), h = std::atoi(argv[2]), frames = std::atoi(argv[3]), spp = std::atoi(argv[4]);
  const float move = (float)std::atof(argv[5]);
  display_params dp;
  dp.tone = std::atoi(argv[6]);
  dp.adapt_up = (float)std::atof(argv[7]);
  dp.adapt_down = (float)std::atof(argv[8]);
  const std::string out = argv[9];
  const size_t n3 = (size_t)w * h * 3;
  // one device allocation: the frame, the linear output (2 x n3 floats), the rgb8 image (n3 bytes)
  float* dev = nullptr;
  if (hipMalloc((void**)&dev, 2 * n3 * sizeof(float) + n3) != hipSuccess) { std::fprintf(stderr, "hipMalloc failed\n"); return 1; }
  int rc = 0;
  try {
    float *fb = dev, *linear = dev + n3;
    uint8_t* rgb8 = reinterpret_cast<uint8_t*>(dev + 2 * n3);
    device_scene scene(cornell());
    display disp(dp);
    std::ofstream file(out, std::ios::binary);
    std::vector<float> host(n3);
    std::vector<uint8_t> bytes(n3);
    auto put = [&](const void* device, size_t size, void* staging) {
      if (hipMemcpy(staging, device, size, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("hipMemcpy failed");
      file.write(reinterpret_cast<const char*>(staging), (std::streamsize)size);
    };
    for (int f = 0; f < frames; f++) {
      const camera cam(point{278 + (float)f * move, 278, -800}, point{278, 278, 0}, vec{0, 1, 0}, 40, (float)w / (float)h, 0, 800, 0, 1);
      const PtRenderParams p{w, h, spp, 50, 0, 1, 0, 0};
      check(pt_render(scene.s, &cam.c, &p, fb, nullptr), "pt_render");
      disp.meter(w, h, fb);
      disp.apply(w, h, fb, rgb8, linear);
      if (disp.frames() != f + 1) throw std::runtime_error("display::frames");
      const float e = disp.exposure();
      const std::array<uint32_t, 257> hist = disp.histogram();
      put(fb, n3 * sizeof(float), host.data());
      put(linear, n3 * sizeof(float), host.data());
      file.write(reinterpret_cast<const char*>(&e), sizeof e);
      file.write(reinterpret_cast<const char*>(hist.data()), sizeof(uint32_t) * hist.size());
      put(rgb8, n3, bytes.data());
    }
    display_params manual = dp;
    manual.ev_bias = 1.0f;
    display_apply(w, h, fb, rgb8, nullptr, manual);
    if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("hipDeviceSynchronize failed");
    put(rgb8, n3, bytes.data());
    disp.reset();
    if (disp.frames() != 0 || disp.exposure() != 0.0f) throw std::runtime_error("display::reset");
    std::printf("%dx%d, %d frames x %d spp, move %g, tone %d, adaptation %g up / %g down: display stage\n", w, h, frames, spp, (double)move, dp.tone,
                (double)dp.adapt_up, (double)dp.adapt_down);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    rc = 1;
  }
  (void)hipFree(dev);
  return rc;
}
