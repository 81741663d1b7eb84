// Stand-alone host check of pixel_footprint (csrc/pt_render.hip: KArgs.foot of the camera rays' candidate cache) for
// tests/test_launch_plan_cpu.py: the launcher's source compiled as HOST code only (hipcc --cuda-host-only -x hip) with
// AddressSanitizer + UBSan on the host side alone, and run directly.  No device call is made.  `before` below is the arithmetic as it stood inside the
// launcher's `launch` lambda before pixel_footprint was factored out of it, kept here line for line as the reference: the eleven values
// must agree bit for bit for the Cornell camera at 1920 x 1080 — and for a camera off the axes, one far from the origin and a 1 x 1 frame.
#include <cstdio>
#include <cstring>

#include "../../path_tracer_amd/csrc/pt_render.hip"

// A host-only compile has no device code to register: the code object the host side expects (its name: -cuid=footprint) is this empty
// bundle, and the registration calls the compiler emits at start-up end here instead of in the HIP runtime, which is never initialised.
extern "C" {
__attribute__((aligned(4096))) const char __hip_fatbin_footprint[32] = "__CLANG_OFFLOAD_BUNDLE__";
void** __hipRegisterFatBinary(const void*) { static void* handle = nullptr; return &handle; }
void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned int, void*, void*, void*, void*, int*) {}
void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}
void __hipUnregisterFatBinary(void**) {}
}

static void before(const Cam& cm, float inv_w, float inv_h, float foot[11]) {
  float base[3], hw[3], vh[3];
  double dmax = 0, lh = 0, lv = 0;
  for (int k = 0; k < 3; k++) {
    base[k] = cm.llc[k] - cm.origin[k]; hw[k] = cm.horizontal[k] * inv_w; vh[k] = cm.vertical[k] * inv_h;
    foot[k] = base[k]; foot[3 + k] = hw[k]; foot[6 + k] = vh[k];
    lh += (double)hw[k] * hw[k]; lv += (double)vh[k] * vh[k];
    dmax += std::fabs((double)cm.llc[k]) + std::fabs((double)cm.origin[k]) + std::fabs((double)cm.horizontal[k]) + std::fabs((double)cm.vertical[k]);
  }
  lh = std::sqrt(lh); lv = std::sqrt(lv);
  foot[9] = (float)((0.5 * (lh + lv)) * 1.001 + 1e-5 * dmax);
  foot[10] = (float)(1e-5 * dmax);
}

struct View { float from[3], at[3], vfov, focus; int w, h; };

int main() {
  const View views[] = {
      {{278, 278, -800}, {278, 278, 0}, 40.0f, 800.0f, 1920, 1080}, // the Cornell camera (path_tracer_amd/scenes.py: cornell_box)
      {{13, 2, 3}, {0.5f, 0.25f, -1}, 20.0f, 10.0f, 400, 225},
      {{1.0e6f, -2.0e6f, 3.0e6f}, {1.0e6f + 3, -2.0e6f, 3.0e6f - 4}, 75.0f, 5.0f, 3840, 2160},
      {{0, 0, 1}, {0, 0, 0}, 90.0f, 1.0f, 1, 1},
  };
  const float vup[3] = {0, 1, 0};
  int bad = 0;
  for (const View& v : views) {
    PtCamera pc;
    if (pt_camera_init(&pc, v.from, v.at, vup, v.vfov, (float)v.w / (float)v.h, 0.0f, v.focus, 0.0f, 1.0f) != PT_OK) return 2;
    Cam cam;
    static_assert(sizeof(Cam) == sizeof(PtCamera), "launch_render copies a PtCamera into KArgs.cam");
    std::memcpy(&cam, &pc, sizeof cam);
    const float inv_w = 1.0f / (float)v.w, inv_h = 1.0f / (float)v.h;
    float want[11], got[12];
    got[11] = -7.0f; // (one past the end stays as it is)
    before(cam, inv_w, inv_h, want);
    pixel_footprint(cam, inv_w, inv_h, got);
    if (std::memcmp(want, got, sizeof want) != 0 || got[11] != -7.0f) {
      bad++;
      for (int k = 0; k < 11; k++) std::printf("%dx%d foot[%d]: %.9g, before %.9g\n", v.w, v.h, k, got[k], want[k]);
    }
    if (&v == &views[0]) { // the headline frame by hand: the viewport at the focus distance is 1035.3 x 582.35 (2 x 800 tan 20 deg high), a pixel
                           // 0.5392 each way; the camera looks along +z, so u = -x; sum of |coordinates| ~ 3 782: rounding term 0.0378
      const float ax = std::fabs(got[3]);
      if (!(got[0] > 517.0f && got[0] < 518.0f && got[2] == 800.0f && ax > 0.539f && ax < 0.540f && got[4] == 0.0f && got[7] > 0.539f && got[7] < 0.540f &&
            got[9] > 0.57f && got[9] < 0.585f && got[10] > 0.037f && got[10] < 0.039f)) {
        bad++;
        for (int k = 0; k < 11; k++) std::printf("cornell foot[%d]: %.9g\n", k, got[k]);
      }
    }
  }
  if (bad) return 1;
  std::printf("FOOTPRINT_OK\n");
  return 0;
}
