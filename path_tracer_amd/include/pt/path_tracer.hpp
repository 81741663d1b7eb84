// path_tracer.hpp — C++20 host facade over the C ABI (include/pt_render.h).
//
// Keeps the reference's scene-description types as the input API surface (same names,
// constructor argument order and meaning; citations into /root/reference/include):
//
//   sphere(cen, r, mat) / sphere(cen0, cen1, t0, t1, r, mat)     sphere.hpp:30,40
//   xy_rect / xz_rect / yz_rect (a0, a1, b0, b1, k, mat)          rectangle.hpp:21,59,97
//   triangle(v0, v1, v2, mat)                                      triangle.hpp:107
//   box(p0, p1, mat)                                               box.hpp:15
//   constant_medium(boundary, density, color | texture)            constant_medium.hpp:18,23
//   lambertian_material / metal_material / dielectric_material /
//   lightsource_material / isotropic_material                      material.hpp:11-131
//   solid_texture / checker_texture / image_texture                texture.hpp:18-152
//   camera(look_from, look_at, vup, vfov, aspect, aperture, focus_dist, t0, t1)   camera.hpp:67-69
//   hittable_t = std::variant<sphere, xy_rect, triangle, box, constant_medium[, xz_rect, yz_rect]>
//                                                                  render.hpp:22-23
//   render<width, height, samples>(frame_buf, hittables, cam)      render.hpp:141-143
//
// The std::variant values never reach the device: flatten() walks them once on the host
// (std::visit) into the tagged tables of PtSceneDesc; pt_scene_create() turns those into the
// 16-byte record runs the kernels read from LDS.  Header-only; link with -lpt_render.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <map>
#include <stdexcept>
#include <string>
#include <tuple>
#include <variant>
#include <vector>

#include "../../../include/pt_render.h"
#include "../../../include/pt_post.h"
#include "../../../include/pt_spatial_variance.h"
#include "../../../include/pt_metrics.h"
#include "../../../include/pt_encode.h"
#include "image_io.hpp"

namespace pt {

using real_t = float; // vec.hpp:8

// Minimal float3 with the accessor names of sycl::float3 (rtweekend.hpp:25-27 aliases it three ways).
struct float3 {
  float v[3]{0, 0, 0};
  constexpr float3() = default;
  constexpr float3(float x, float y, float z) : v{x, y, z} {}
  constexpr float x() const { return v[0]; }
  constexpr float y() const { return v[1]; }
  constexpr float z() const { return v[2]; }
  friend bool operator==(const float3& a, const float3& b) { return a.v[0] == b.v[0] && a.v[1] == b.v[1] && a.v[2] == b.v[2]; }
  friend bool operator<(const float3& a, const float3& b) { return std::tie(a.v[0], a.v[1], a.v[2]) < std::tie(b.v[0], b.v[1], b.v[2]); }
};
using point = float3;
using color = float3;
using vec = float3;

class pt_error : public std::runtime_error {
 public:
  pt_error(int code, const std::string& where)
      : std::runtime_error(where + ": " + pt_error_string(code) + " (" + pt_last_error() + ")"), code(code) {}
  int code;
};
inline void check(int rc, const char* where) {
  if (rc != PT_OK) throw pt_error(rc, where);
}

// ---- textures (texture.hpp) ------------------------------------------------------------------
struct solid_texture {
  solid_texture() = default;
  solid_texture(const color& c) : color_value{c} {}
  solid_texture(float r, float g, float b) : color_value{r, g, b} {}
  color color_value;
  auto key() const { return std::tie(color_value); }
};
struct checker_texture {
  checker_texture() = default;
  checker_texture(const solid_texture& x, const solid_texture& y) : odd{x}, even{y} {} // texture.hpp:35
  checker_texture(const color& c1, const color& c2) : odd{c1}, even{c2} {}              // texture.hpp:38
  solid_texture odd, even;
  auto key() const { return std::tie(odd.color_value, even.color_value); }
};
// The atlas behind image_texture (texture.hpp:71,157): starts with the {0,0,1} fallback texel.
struct texture_atlas {
  std::vector<uint8_t> data{0, 0, 1};
};
inline texture_atlas& default_atlas() {
  static texture_atlas a;
  return a;
}
struct image_texture {
  // texture.hpp:97-117 with the decode step left to the caller (stb is not a dependency here):
  // `rgb` is height*width*3 bytes, rows top-down.
  static image_texture from_rgb8(const uint8_t* rgb, std::size_t width, std::size_t height, float cyclic_frequency = 1.f,
                                 texture_atlas& atlas = default_atlas()) {
    image_texture t;
    if (!rgb || !width || !height) return t; // load failure: 1x1 texture at the fallback texel (texture.hpp:106-111)
    t.width = width; t.height = height; t.cyclic_frequency = cyclic_frequency;
    t.offset = atlas.data.size() / 3;
    atlas.data.insert(atlas.data.end(), rgb, rgb + width * height * 3);
    return t;
  }
  // texture.hpp:97-117: load an image file and append its texels to the atlas.  stb_image is not a dependency of this host: PNG,
  // baseline JPEG and binary PPM are decoded by pt/image_io.hpp (the reference's own images/Xilinx.jpg and images/SYCL.png load as
  // main.cpp:133,145 load them; the decoded texels are the ones the Python host's loader produces — image_io.hpp says which
  // decoder choices that pins).  Everything else keeps the reference's failure semantics (texture.hpp:106-111): a message on
  // stderr and the 1x1 texture at offset 0, i.e. the {0,0,1} fallback texel the atlas starts with; never an exception.
  static image_texture image_texture_factory(const char* file_name, float cyclic_frequency = 1.f,
                                             texture_atlas& atlas = default_atlas()) {
    image_io::Image img;
    const char* reason = image_io::load_rgb8(file_name, img);
    if (reason) {
      std::cerr << "ERROR: Could not load texture image file '" << (file_name ? file_name : "(null)") << "'.\n" << reason << std::endl;
      image_texture t;
      t.cyclic_frequency = cyclic_frequency; // texture.hpp:116: w = h = 1, offset 0, the caller's frequency
      return t;
    }
    return from_rgb8(img.rgb.data(), img.width, img.height, cyclic_frequency, atlas);
  }
  std::size_t width{1}, height{1}, offset{0};
  float cyclic_frequency{1.f};
  auto key() const { return std::tie(width, height, offset, cyclic_frequency); }

};
using texture_t = std::variant<checker_texture, solid_texture, image_texture>; // texture.hpp:154

// ---- materials (material.hpp) ------------------------------------------------------------------
struct lambertian_material {
  lambertian_material() = default;
  lambertian_material(const color& a) : albedo{solid_texture{a}} {}
  lambertian_material(const texture_t& a) : albedo{a} {}
  texture_t albedo;
};
struct metal_material {
  metal_material() = default;
  metal_material(const color& a, float f) : albedo{a}, fuzz{std::clamp(f, 0.0f, 1.0f)} {} // material.hpp:35-37
  color albedo;
  float fuzz{0};
};
struct dielectric_material {
  dielectric_material() = default;
  dielectric_material(real_t ri, const color& albedo) : ref_idx{ri}, albedo{albedo} {}
  real_t ref_idx{1};
  color albedo;
};
struct lightsource_material {
  lightsource_material() = default;
  lightsource_material(const texture_t& a) : emit{a} {}
  lightsource_material(const color& a) : emit{solid_texture{a}} {}
  texture_t emit;
};
struct isotropic_material {
  isotropic_material(const color& a) : albedo{solid_texture{a}} {}
  isotropic_material(const texture_t& a) : albedo{a} {}
  texture_t albedo;
};
using material_t = std::variant<lambertian_material, metal_material, dielectric_material, lightsource_material,
                                isotropic_material>; // material.hpp:133-135

// ---- hittables ------------------------------------------------------------------------------------
struct sphere {
  sphere() = default;
  sphere(const point& cen, real_t r, const material_t& m) : center0{cen}, center1{cen}, radius{r}, time0{0}, time1{0}, material_type{m} {}
  sphere(const point& cen0, const point& cen1, real_t t0, real_t t1, real_t r, const material_t& m)
      : center0{cen0}, center1{cen1}, radius{r}, time0{t0}, time1{t1}, material_type{m} {}
  point center0, center1;
  real_t radius{0}, time0{0}, time1{0};
  material_t material_type;
};
struct xy_rect {
  xy_rect() = default;
  xy_rect(real_t x0, real_t x1, real_t y0, real_t y1, real_t k, const material_t& m) : x0{x0}, x1{x1}, y0{y0}, y1{y1}, k{k}, material_type{m} {}
  real_t x0{}, x1{}, y0{}, y1{}, k{};
  material_t material_type;
};
struct xz_rect {
  xz_rect() = default;
  xz_rect(real_t x0, real_t x1, real_t z0, real_t z1, real_t k, const material_t& m) : x0{x0}, x1{x1}, z0{z0}, z1{z1}, k{k}, material_type{m} {}
  real_t x0{}, x1{}, z0{}, z1{}, k{};
  material_t material_type;
};
struct yz_rect {
  yz_rect() = default;
  yz_rect(real_t y0, real_t y1, real_t z0, real_t z1, real_t k, const material_t& m) : y0{y0}, y1{y1}, z0{z0}, z1{z1}, k{k}, material_type{m} {}
  real_t y0{}, y1{}, z0{}, z1{}, k{};
  material_t material_type;
};
// triangle.hpp:102-122: _triangle<IntersectionStrategy>; `triangle` = the Moller-Trumbore default (what main.cpp builds),
// `badouel_triangle` = _triangle<badouel_ray_triangle_intersec> (triangle.hpp:14-56).
template <int Strategy = PT_TRI_MOLLER_TRUMBORE>
struct _triangle {
  _triangle() = default;
  _triangle(const point& v0, const point& v1, const point& v2, const material_t& m) : v0{v0}, v1{v1}, v2{v2}, material_type{m} {}
  point v0, v1, v2;
  material_t material_type;
  static constexpr int strategy = Strategy;
};
using triangle = _triangle<>;
using badouel_triangle = _triangle<PT_TRI_BADOUEL>;
struct box {
  box() = default;
  box(const point& p0, const point& p1, const material_t& m) : box_min{p0}, box_max{p1}, material_type{m} {}
  point box_min, box_max;
  material_t material_type;
};
using hittableVolume_t = std::variant<sphere, box>; // constant_medium.hpp:10
struct constant_medium {
  constant_medium(const hittableVolume_t& b, real_t d, const texture_t& a) : boundary{b}, neg_inv_density{-1 / d}, phase_function{isotropic_material{a}} {}
  constant_medium(const hittableVolume_t& b, real_t d, const color& a) : boundary{b}, neg_inv_density{-1 / d}, phase_function{isotropic_material{a}} {}
  hittableVolume_t boundary;
  real_t neg_inv_density;
  material_t phase_function;
};
// The reference's five alternatives first (same indices); xz_rect/yz_rect and the Badouel-strategy triangle are extensions.
using hittable_t = std::variant<sphere, xy_rect, triangle, box, constant_medium, xz_rect, yz_rect, badouel_triangle>;

// ---- camera (camera.hpp:67-87) -----------------------------------------------------------------------
class camera {
 public:
  camera(const point& look_from, const point& look_at, const vec& vup, real_t degree_vfov, real_t aspect_ratio,
         real_t aperture, real_t focus_dist, real_t time0 = 0, real_t time1 = 0) {
    check(pt_camera_init(&c, look_from.v, look_at.v, vup.v, degree_vfov, aspect_ratio, aperture, focus_dist, time0, time1),
          "pt_camera_init");
  }
  PtCamera c{};
};

// ---- flattening the variants into the C-ABI tables ------------------------------------------------------
struct scene_tables {
  std::vector<PtHittable> hittables;
  std::vector<PtMaterial> materials;
  std::vector<PtTexture> textures;
  std::vector<uint8_t> atlas;
  PtSceneDesc desc() const {
    PtSceneDesc d{};
    d.hittables = hittables.data(); d.n_hittables = (int32_t)hittables.size();
    d.materials = materials.data(); d.n_materials = (int32_t)materials.size();
    d.textures = textures.data(); d.n_textures = (int32_t)textures.size();
    d.atlas = atlas.empty() ? nullptr : atlas.data(); d.atlas_bytes = atlas.size();
    return d;
  }
};

namespace detail {
inline void put3(float* d, const float3& s) { d[0] = s.v[0]; d[1] = s.v[1]; d[2] = s.v[2]; }

struct flattener {
  scene_tables& out;
  bool uses_image = false;
  // value-equal textures / materials share one table entry (same rule as the Python packer)
  std::map<std::tuple<int, std::array<float, 7>, std::array<uint64_t, 3>>, int> tex_ids;
  std::map<std::tuple<int, int, std::array<float, 4>>, int> mat_ids;

  int texture(const texture_t& t) {
    PtTexture e{};
    std::array<float, 7> f{};
    std::array<uint64_t, 3> u{};
    e.kind = (int32_t)t.index(); // variant order == ABI tag order (texture.hpp:154)
    if (auto* s = std::get_if<solid_texture>(&t)) {
      put3(e.color0, s->color_value);
    } else if (auto* c = std::get_if<checker_texture>(&t)) {
      put3(e.color0, c->odd.color_value); put3(e.color1, c->even.color_value);
    } else {
      auto& i = std::get<image_texture>(t);
      e.width = (uint32_t)i.width; e.height = (uint32_t)i.height; e.offset = (uint32_t)i.offset; e.freq = i.cyclic_frequency;
      u = {i.width, i.height, i.offset};
      uses_image = true;
    }
    std::copy(e.color0, e.color0 + 3, f.begin()); std::copy(e.color1, e.color1 + 3, f.begin() + 3); f[6] = e.freq;
    auto key = std::make_tuple(e.kind, f, u);
    auto it = tex_ids.find(key);
    if (it != tex_ids.end()) return it->second;
    out.textures.push_back(e);
    return tex_ids[key] = (int)out.textures.size() - 1;
  }

  int material(const material_t& m) {
    PtMaterial e{};
    e.kind = (int32_t)m.index(); // variant order == ABI tag order (material.hpp:133-135)
    e.texture = -1;
    std::visit([&](auto&& a) {
      using T = std::decay_t<decltype(a)>;
      if constexpr (std::is_same_v<T, lambertian_material> || std::is_same_v<T, isotropic_material>) e.texture = texture(a.albedo);
      else if constexpr (std::is_same_v<T, lightsource_material>) e.texture = texture(a.emit);
      else if constexpr (std::is_same_v<T, metal_material>) { put3(e.color, a.albedo); e.param = a.fuzz; }
      else { put3(e.color, a.albedo); e.param = a.ref_idx; }
    }, m);
    auto key = std::make_tuple(e.kind, e.texture, std::array<float, 4>{e.color[0], e.color[1], e.color[2], e.param});
    auto it = mat_ids.find(key);
    if (it != mat_ids.end()) return it->second;
    out.materials.push_back(e);
    return mat_ids[key] = (int)out.materials.size() - 1;
  }

  static void fill(float* f, const sphere& s) { put3(f, s.center0); put3(f + 3, s.center1); f[6] = s.radius; f[7] = s.time0; f[8] = s.time1; }
  static void fill(float* f, const box& b) { put3(f, b.box_min); put3(f + 3, b.box_max); }

  void hittable(const hittable_t& h) {
    PtHittable e{};
    std::visit([&](auto&& a) {
      using T = std::decay_t<decltype(a)>;
      if constexpr (std::is_same_v<T, sphere>) { e.kind = PT_HIT_SPHERE; e.material = material(a.material_type); fill(e.f, a); }
      else if constexpr (std::is_same_v<T, xy_rect>) { e.kind = PT_HIT_XY_RECT; e.material = material(a.material_type); float v[5] = {a.x0, a.x1, a.y0, a.y1, a.k}; std::copy(v, v + 5, e.f); }
      else if constexpr (std::is_same_v<T, xz_rect>) { e.kind = PT_HIT_XZ_RECT; e.material = material(a.material_type); float v[5] = {a.x0, a.x1, a.z0, a.z1, a.k}; std::copy(v, v + 5, e.f); }
      else if constexpr (std::is_same_v<T, yz_rect>) { e.kind = PT_HIT_YZ_RECT; e.material = material(a.material_type); float v[5] = {a.y0, a.y1, a.z0, a.z1, a.k}; std::copy(v, v + 5, e.f); }
      else if constexpr (std::is_same_v<T, triangle> || std::is_same_v<T, badouel_triangle>) {
        e.kind = PT_HIT_TRIANGLE; e.strategy = T::strategy; e.material = material(a.material_type);
        put3(e.f, a.v0); put3(e.f + 3, a.v1); put3(e.f + 6, a.v2);
      }
      else if constexpr (std::is_same_v<T, box>) { e.kind = PT_HIT_BOX; e.material = material(a.material_type); fill(e.f, a); }
      else {
        e.kind = PT_HIT_CONSTANT_MEDIUM; e.material = material(a.phase_function);
        if (auto* s = std::get_if<sphere>(&a.boundary)) { e.boundary_kind = PT_HIT_SPHERE; fill(e.f, *s); }
        else { e.boundary_kind = PT_HIT_BOX; fill(e.f, std::get<box>(a.boundary)); }
        e.f[9] = a.neg_inv_density;
      }
    }, h);
    out.hittables.push_back(e);
  }
};
} // namespace detail

inline scene_tables flatten(const std::vector<hittable_t>& hittables, const texture_atlas& atlas = default_atlas()) {
  scene_tables t;
  detail::flattener f{t};
  for (auto& h : hittables) f.hittable(h); // list order == traversal order (render.hpp:37)
  if (f.uses_image) t.atlas = atlas.data;
  return t;
}

// Device-resident scene; RAII over pt_scene_create / pt_scene_destroy.
class device_scene {
 public:
  explicit device_scene(const std::vector<hittable_t>& hittables, const texture_atlas& atlas = default_atlas()) {
    scene_tables t = flatten(hittables, atlas);
    PtSceneDesc d = t.desc();
    check(pt_scene_create(&d, &s), "pt_scene_create");
  }
  ~device_scene() { pt_scene_destroy(s); }
  device_scene(const device_scene&) = delete;
  device_scene& operator=(const device_scene&) = delete;
  PtScene* s = nullptr;
};

// frame buffer [height][width] of color, y = 0 is the bottom scan-line (render.hpp:105, main.cpp:41)
using frame_buffer = std::vector<color>;

// render.hpp:141-160 with run-time sizes; depth 50 as render.hpp:144.
inline void render(int width, int height, int samples, frame_buffer& frame_buf, const std::vector<hittable_t>& hittables,
                   const camera& cam, int depth = 50) {
  device_scene scene(hittables);
  PtRenderParams p{width, height, samples, depth, 0, 1, 0, 0};
  frame_buf.resize((std::size_t)width * height);
  static_assert(sizeof(color) == 12);
  check(pt_render_host(scene.s, &cam.c, &p, reinterpret_cast<float*>(frame_buf.data())), "pt_render_host");
}

// The reference's call shape: render<width, height, samples>(frame_buf, hittables, cam).
template <int width, int height, int samples>
void render(frame_buffer& frame_buf, std::vector<hittable_t>& hittables, camera& cam) {
  render(width, height, samples, frame_buf, hittables, cam);
}

// First-hit feature buffers (include/pt_render.h: pt_render_aov) — guide images for a denoiser, mattes for compositing: the render at
// depth 1 with the first bounce's record kept, `samples` camera rays per pixel from the pixel's own stream, a pass that needs nothing
// from render().  The planes are DEVICE buffers the caller owns, as in the C ABI (this header does no device allocation): albedo, normal,
// direct hold aov_plane_elems(..., 3) floats, laid out like render()'s frame buffer; depth, coverage and id aov_plane_elems(..., 1)
// elements, [height][width] ([local tile][64] for shards).  nullptr = plane not wanted.
struct aov_buffers {
  float* albedo = nullptr;
  float* normal = nullptr;
  float* direct = nullptr;
  float* depth = nullptr;
  float* coverage = nullptr;
  int32_t* id = nullptr;
};
inline int64_t aov_plane_elems(int width, int height, int channels, int shard_index = 0, int shard_count = 1) {
  const PtRenderParams p{width, height, 1, 1, shard_index, shard_count, 0, 0};
  return pt_aov_plane_elems(&p, channels);
}
// asynchronous on `stream` (the scene must outlive the pass)
inline void render_aov(int width, int height, int samples, const aov_buffers& planes, const device_scene& scene, const camera& cam,
                       int shard_index = 0, int shard_count = 1, void* stream = nullptr) {
  const PtRenderParams p{width, height, samples, 1, shard_index, shard_count, 0, 0};
  const PtAovBuffers b{(int32_t)sizeof(PtAovBuffers), 0, planes.albedo, planes.normal, planes.direct, planes.depth, planes.coverage, planes.id};
  check(pt_render_aov(scene.s, &cam.c, &p, &b, stream), "pt_render_aov");
}
// from a list of hittables: the planes are complete on return (the temporary scene's release waits for the device)
inline void render_aov(int width, int height, int samples, const aov_buffers& planes, const std::vector<hittable_t>& hittables,
                       const camera& cam, int shard_index = 0, int shard_count = 1) {
  device_scene scene(hittables);
  render_aov(width, height, samples, planes, scene, cam, shard_index, shard_count, nullptr);
}

// The edge-avoiding a-trous denoiser over a finished whole frame (include/pt_render.h: pt_denoise), guided by render_aov's planes.
// color, out ([height][width][3]; out may be color), the optional guides albedo, normal ([height][width][3]) and depth ([height][width])
// and scratch (denoise_scratch_floats(width, height) floats, 16-byte aligned) are DEVICE buffers the caller owns; a sigma <= 0 turns
// its term off.  The defaults are the header's (pt_denoise_params_init).
struct denoise_params {
  int iterations = PT_DENOISE_DEFAULT_ITERATIONS;
  float sigma_color = PT_DENOISE_DEFAULT_SIGMA_COLOR, sigma_normal = PT_DENOISE_DEFAULT_SIGMA_NORMAL;
  float sigma_depth = PT_DENOISE_DEFAULT_SIGMA_DEPTH, sigma_albedo = PT_DENOISE_DEFAULT_SIGMA_ALBEDO;
  bool demodulate = true; // filter color / (albedo + 1e-3) and multiply the albedo back: needs the albedo plane
};
inline int64_t denoise_scratch_floats(int width, int height) { return pt_denoise_scratch_floats(width, height); }
// asynchronous on `stream`
inline void denoise(int width, int height, const float* color, const float* albedo, const float* normal, const float* depth, float* out,
                    float* scratch, const denoise_params& dp = {}, void* stream = nullptr) {
  const PtDenoiseParams p{(int32_t)sizeof(PtDenoiseParams), width, height, dp.iterations, dp.sigma_color, dp.sigma_normal, dp.sigma_depth,
                          dp.sigma_albedo, dp.demodulate ? PT_DENOISE_DEMODULATE : 0u, 0};
  check(pt_denoise(&p, color, albedo, normal, depth, out, scratch, stream), "pt_denoise");
}

// The variance-guided denoiser (include/pt_render.h: pt_variance_denoise): denoise() with the colour tolerance taken per pixel from
// `variance` ([height][width][3], the variance of each pixel's mean: accumulator::variance, or any other estimate), so that one setting
// fits every sample count of an adaptive frame.  The buffers are DEVICE buffers the caller owns, as for denoise(); out may be color,
// variance_out (optional: the filtered frame's residual variance) may be variance; scratch: variance_denoise_scratch_floats(width,
// height) floats, 16-byte aligned.  The defaults are the header's (pt_variance_denoise_params_init).
struct variance_denoise_params {
  int iterations = PT_VDENOISE_DEFAULT_ITERATIONS;
  float sigma_variance = PT_VDENOISE_DEFAULT_SIGMA_VARIANCE, sigma_normal = PT_VDENOISE_DEFAULT_SIGMA_NORMAL;
  float sigma_depth = PT_VDENOISE_DEFAULT_SIGMA_DEPTH, sigma_albedo = PT_VDENOISE_DEFAULT_SIGMA_ALBEDO;
  bool demodulate = true; // filter color / (albedo + 1e-3) and multiply the albedo back: needs the albedo plane
};
inline int64_t variance_denoise_scratch_floats(int width, int height) { return pt_variance_denoise_scratch_floats(width, height); }
// asynchronous on `stream`
inline void variance_denoise(int width, int height, const float* color, const float* variance, const float* albedo, const float* normal,
                             const float* depth, float* out, float* variance_out, float* scratch, const variance_denoise_params& dp = {},
                             void* stream = nullptr) {
  const PtVarianceDenoiseParams p{(int32_t)sizeof(PtVarianceDenoiseParams), width, height, dp.iterations, dp.sigma_variance, dp.sigma_normal,
                                  dp.sigma_depth, dp.sigma_albedo, dp.demodulate ? PT_VDENOISE_DEMODULATE : 0u, 0};
  check(pt_variance_denoise(&p, color, variance, albedo, normal, depth, out, variance_out, scratch, stream), "pt_variance_denoise");
}

// Temporal reprojection (include/pt_render.h: PtTemporal): the history of one image sequence, RAII over pt_temporal_create /
// pt_temporal_destroy.  push() blends a frame into the history fetched through the previous push's camera and rejected by the guides
// (depth: required; normal, id: optional) — render_aov's planes for the frame's camera.  The planes are DEVICE buffers the caller owns,
// [height][width](x3); out_color may be color, out_variance may be variance_in; variance_in, out_variance and out_history are optional.
// The defaults are the header's (pt_temporal_params_init).
struct temporal_params {
  float alpha = PT_TEMPORAL_DEFAULT_ALPHA, tol_depth = PT_TEMPORAL_DEFAULT_TOL_DEPTH, tol_normal = PT_TEMPORAL_DEFAULT_TOL_NORMAL;
};
class temporal {
 public:
  temporal(int width, int height) { check(pt_temporal_create(width, height, &t_), "pt_temporal_create"); }
  ~temporal() { pt_temporal_destroy(t_); }
  temporal(const temporal&) = delete;
  temporal& operator=(const temporal&) = delete;
  // asynchronous on `stream`
  void push(const camera& cam, const float* color, const float* depth, const float* normal, const int32_t* id, const float* variance_in,
            float* out_color, float* out_variance = nullptr, float* out_history = nullptr, const temporal_params& tp = {},
            void* stream = nullptr) {
    const PtTemporalParams p{(int32_t)sizeof(PtTemporalParams), tp.alpha, tp.tol_depth, tp.tol_normal, 0u, {0, 0, 0}};
    check(pt_temporal_push(t_, &p, &cam.c, color, depth, normal, id, variance_in, out_color, out_variance, out_history, stream), "pt_temporal_push");
  }
  void reset(void* stream = nullptr) { check(pt_temporal_reset(t_, stream), "pt_temporal_reset"); }
  int frames() const { return pt_temporal_frames(t_); }
  PtTemporal* handle() const { return t_; }

 private:
  PtTemporal* t_ = nullptr;
};

// The display stage (include/pt_render.h: PtDisplay): a luminance histogram metered on the device, an exposure solved from it with eye
// adaptation across the frames of a sequence, and exposure + tone curve + the output stage's quantiser in one pass; RAII over
// pt_display_create / pt_display_destroy.  color and linear_out are DEVICE buffers [height][width][3] (the frame buffer's layout), rgb8_out
// is [height][width][3] bytes with row 0 = top; either output may be null, linear_out may be color.  The defaults are the header's
// (pt_display_params_init).  display_apply() is the stateless form: the exposure is dp.ev_bias.
struct display_params {
  int tone = PT_DISPLAY_DEFAULT_TONE; // PT_TONE_REFERENCE, PT_TONE_REINHARD, PT_TONE_ACES
  float ev_bias = PT_DISPLAY_DEFAULT_EV_BIAS, ev_min = PT_DISPLAY_DEFAULT_EV_MIN, ev_max = PT_DISPLAY_DEFAULT_EV_MAX;
  int lo_permille = PT_DISPLAY_DEFAULT_LO_PERMILLE, hi_permille = PT_DISPLAY_DEFAULT_HI_PERMILLE;
  float adapt_up = PT_DISPLAY_DEFAULT_ADAPT_UP, adapt_down = PT_DISPLAY_DEFAULT_ADAPT_DOWN;
  float white = PT_DISPLAY_DEFAULT_WHITE;
  int rect[4] = {0, 0, 0, 0}; // x0, y0, x1, y1 of the metering rectangle; four zeros: the whole frame
  PtDisplayParams c() const {
    return PtDisplayParams{(int32_t)sizeof(PtDisplayParams), tone, 0u, ev_bias, ev_min, ev_max, lo_permille, hi_permille, adapt_up, adapt_down,
                           white, rect[0], rect[1], rect[2], rect[3], 0};
  }
};
inline void display_apply(int width, int height, const float* color, uint8_t* rgb8_out, float* linear_out = nullptr,
                          const display_params& dp = {}, void* stream = nullptr) {
  const PtDisplayParams p = dp.c();
  check(pt_display_apply(nullptr, &p, color, width, height, rgb8_out, linear_out, stream), "pt_display_apply");
}
class display {
 public:
  explicit display(const display_params& dp = {}) : params(dp) { check(pt_display_create(&d_), "pt_display_create"); }
  ~display() { pt_display_destroy(d_); }
  display(const display&) = delete;
  display& operator=(const display&) = delete;
  // asynchronous on `stream`: histogram, solve and adaptation
  void meter(int width, int height, const float* color, void* stream = nullptr) {
    const PtDisplayParams p = params.c();
    check(pt_display_meter(d_, &p, color, width, height, stream), "pt_display_meter");
  }
  // asynchronous on `stream`: the exposure is the state's
  void apply(int width, int height, const float* color, uint8_t* rgb8_out, float* linear_out = nullptr, void* stream = nullptr) const {
    const PtDisplayParams p = params.c();
    check(pt_display_apply(d_, &p, color, width, height, rgb8_out, linear_out, stream), "pt_display_apply");
  }
  void set_exposure(float ev, void* stream = nullptr) { check(pt_display_set_exposure(d_, ev, stream), "pt_display_set_exposure"); }
  void reset(void* stream = nullptr) { check(pt_display_reset(d_, stream), "pt_display_reset"); }
  int frames() const { return pt_display_frames(d_); }
  // these two synchronise `stream`
  float exposure(void* stream = nullptr) const {
    float ev = 0.0f;
    check(pt_display_exposure(d_, &ev, stream), "pt_display_exposure");
    return ev;
  }
  std::array<uint32_t, 257> histogram(void* stream = nullptr) const {
    std::array<uint32_t, 257> h{};
    check(pt_display_histogram(d_, h.data(), stream), "pt_display_histogram");
    return h;
  }
  PtDisplay* handle() const { return d_; }
  display_params params;

 private:
  PtDisplay* d_ = nullptr;
};

// The firefly stage (include/pt_post.h: pt_firefly), before the filters: a pixel whose luminance exceeds k times the largest (rank 1) or
// second largest (rank 2) luminance among its up to eight neighbours is scaled down to that; with `repair` a pixel that is not finite
// becomes the mean of its finite neighbours.  The clamp is BIASED (it only removes energy): nothing applies it unless asked.  color, out
// and the optional variance, variance_out ([height][width][3]) and counts (uint32[2]: clamped, repaired) are DEVICE buffers the caller
// owns; out must not overlap color, variance_out may be variance.  The defaults are the header's (pt_firefly_params_init).
struct firefly_params {
  int rank = PT_FIREFLY_DEFAULT_RANK;
  float k = PT_FIREFLY_DEFAULT_K;
  bool repair = true;
};
// asynchronous on `stream`
inline void firefly(int width, int height, const float* color, const float* variance, float* out, float* variance_out = nullptr,
                    uint32_t* counts = nullptr, const firefly_params& fp = {}, void* stream = nullptr) {
  const PtFireflyParams p{(int32_t)sizeof(PtFireflyParams), width, height, fp.rank, fp.k, fp.repair ? PT_FIREFLY_REPAIR : 0u, {0, 0}};
  check(pt_firefly(&p, color, variance, out, variance_out, counts, stream), "pt_firefly");
}

// The spatial variance estimate (include/pt_spatial_variance.h: pt_spatial_variance): the variance of each pixel's mean from the squared
// differences of adjacent pixels in a (2 radius + 1)^2 window, over the pixels that lie on the centre's surface by the guides.  With
// `variance_in` it fills only the pixels that have no estimate (a channel that is not >= 0 and finite) and keeps the others bit for bit;
// without, it makes the whole plane.  color, variance_out and the optional albedo, normal, variance_in ([height][width][3]), depth, id
// ([height][width]) and counts (uint32[2]: estimated, holes) are DEVICE buffers the caller owns; variance_out may be variance_in.  The
// defaults are the header's (pt_spatial_variance_params_init); demodulate < 0: where albedo is given.
struct spatial_variance_params {
  int radius = PT_SVAR_DEFAULT_RADIUS;
  int min_pairs = PT_SVAR_DEFAULT_MIN_PAIRS;
  float tol_depth = PT_SVAR_DEFAULT_TOL_DEPTH;
  float tol_normal = PT_SVAR_DEFAULT_TOL_NORMAL;
  int demodulate = -1; // 0: off, 1: on (needs albedo), -1: on where albedo is given
};
struct spatial_variance_guides {
  const float* albedo = nullptr;
  const float* normal = nullptr;
  const float* depth = nullptr;
  const int32_t* id = nullptr;
};
// asynchronous on `stream`
inline void spatial_variance(int width, int height, const float* color, const spatial_variance_guides& g, const float* variance_in,
                             float* variance_out, uint32_t* counts = nullptr, const spatial_variance_params& sp = {}, void* stream = nullptr) {
  const bool demodulate = sp.demodulate < 0 ? g.albedo != nullptr : sp.demodulate != 0;
  const PtSpatialVarianceParams p{(int32_t)sizeof(PtSpatialVarianceParams), width, height, sp.radius, sp.min_pairs, sp.tol_depth, sp.tol_normal,
                                  demodulate ? PT_SVAR_DEMODULATE : 0u, {0, 0}};
  check(pt_spatial_variance(&p, color, g.albedo, g.normal, g.depth, g.id, variance_in, variance_out, counts, stream), "pt_spatial_variance");
}

// The image error (include/pt_metrics.h: pt_image_error): frame `a` against frame `ref` inside `rect`; each sum is the exact sum of its
// terms rounded once to binary64, whatever the order in which the device adds.  a, ref ([height][width][3]), the optional error_plane
// ([height][width]), `result` (a DEVICE PtImageErrorResult, 8-byte aligned) and `scratch` (image_error_scratch_bytes() bytes, 8-byte
// aligned) are DEVICE buffers the caller owns.  Nothing is read back: copy `result` into an image_error_result when the numbers are wanted.
struct image_error_params {
  int rect[4] = {0, 0, 0, 0}; // x0, y0, x1, y1; four zeros: the whole frame
  double eps = PT_IMAGE_ERROR_DEFAULT_EPS;
  bool no_lds = false;        // the A/B switch PT_IMAGE_ERROR_NO_LDS (the same bits)
};
// The result on the host, with the derived figures: ordinary binary64 host arithmetic on the sums, in the order the header writes.
struct image_error_result : PtImageErrorResult {
  static double mean(const double v[3], uint64_t n) { return n ? ((v[0] + v[1]) + v[2]) / (3.0 * (double)n) : std::nan(""); }
  double mse() const { return mean(sum_sq, pixels); }
  double mae() const { return mean(sum_abs, pixels); }
  double rel_mse() const { return mean(sum_rel, pixels); }
  double psnr(double peak = 1.0) const {
    const double m = mse();
    return m != m ? m : m == 0.0 ? HUGE_VAL : 10.0 * std::log10(peak * peak / m);
  }
};
inline size_t image_error_scratch_bytes() { return (size_t)pt_image_error_scratch_bytes(); }
// asynchronous on `stream`
inline void image_error(int width, int height, const float* a, const float* ref, PtImageErrorResult* result, void* scratch,
                        float* error_plane = nullptr, const image_error_params& ip = {}, void* stream = nullptr) {
  PtImageErrorParams p;
  pt_image_error_params_init(&p, width, height);
  p.rect_x0 = ip.rect[0]; p.rect_y0 = ip.rect[1]; p.rect_x1 = ip.rect[2]; p.rect_y1 = ip.rect[3];
  p.eps = ip.eps;
  p.flags = ip.no_lds ? PT_IMAGE_ERROR_NO_LDS : 0u;
  p.scratch_bytes = pt_image_error_scratch_bytes();
  check(pt_image_error(&p, a, ref, result, error_plane, scratch, stream), "pt_image_error");
}

// The encode stage (include/pt_encode.h: pt_encode, pt_display_encode): linear light -> 8-bit codes by the exact sRGB transfer (the code
// of the real sRGB function, correctly rounded, for every binary32 value), optionally with the 8 x 8 ordered dither in linear light; or
// the reference's quantiser (PT_TRANSFER_REFERENCE: pt_tonemap_rgb8's bytes).  linear / color ([height][width][3] float, row 0 = bottom)
// and rgb8_out ([height][width][3] bytes, row 0 = top) are DEVICE buffers the caller owns and must not overlap.  The defaults are the
// header's (pt_encode_params_init).  display_encode() is display_apply()'s exposure and curve and encode() in one pass: `d` null is the
// stateless form (the exposure is dp.ev_bias).
struct encode_params {
  int transfer = PT_ENCODE_DEFAULT_TRANSFER; // PT_TRANSFER_REFERENCE, PT_TRANSFER_SRGB
  bool dither = false;
  int phase_x = 0, phase_y = 0;              // the dither pattern's offset in pixels
  bool no_vec = false;                       // the A/B switch PT_ENCODE_NO_VEC (the same bits)
  PtEncodeParams c(int width, int height) const {
    return PtEncodeParams{(int32_t)sizeof(PtEncodeParams), width, height, transfer,
                          (dither ? PT_ENCODE_DITHER : 0u) | (no_vec ? PT_ENCODE_NO_VEC : 0u), phase_x, phase_y, 0};
  }
};
// asynchronous on `stream`
inline void encode(int width, int height, const float* linear, uint8_t* rgb8_out, const encode_params& ep = {}, void* stream = nullptr) {
  const PtEncodeParams p = ep.c(width, height);
  check(pt_encode(&p, linear, rgb8_out, stream), "pt_encode");
}
// asynchronous on `stream`
inline void display_encode(int width, int height, const float* color, uint8_t* rgb8_out, const display_params& dp = {},
                           const encode_params& ep = {}, const display* d = nullptr, void* stream = nullptr) {
  const PtDisplayParams p = dp.c();
  const PtEncodeParams e = ep.c(width, height);
  check(pt_display_encode(d ? d->handle() : nullptr, &p, &e, color, rgb8_out, stream), "pt_display_encode");
}

// Progressive rendering: one frame in sample windows; RAII over pt_accum_create / pt_accum_destroy (include/pt_render.h, PtAccum).
// After windows totalling N samples, resolve() holds the bits render() gives at samples = N.  The scene must outlive the accumulator;
// windows run on the default stream (or `stream`) and are ordered like renders of the scene.
//
// Adaptive sampling (pt_adaptive_*): constructed with pt::adaptive, the accumulator keeps a sample count per pixel; add() takes a mask
// and each pixel resolves to the bits render() gives at its own count.  Masks, counts and errors are DEVICE buffers of one element per
// pixel ([height][width]; [local tile][64] for shards) that the caller owns, as in the C ABI: this header does no device allocation.
struct adaptive_t {};
inline constexpr adaptive_t adaptive{};

class accumulator {
 public:
  accumulator(const device_scene& scene, const camera& cam, int width, int height, int depth = 50, uint32_t flags = 0, int shard_index = 0,
              int shard_count = 1)
      : cam_(cam.c), p_{width, height, 1, depth, shard_index, shard_count, flags, 0} {
    check(pt_accum_create(scene.s, &p_, &a_), "pt_accum_create");
  }
  accumulator(adaptive_t, const device_scene& scene, const camera& cam, int width, int height, int depth = 50, uint32_t flags = 0,
              int shard_index = 0, int shard_count = 1)
      : cam_(cam.c), p_{width, height, 1, depth, shard_index, shard_count, flags, 0}, adaptive_(true) {
    check(pt_adaptive_create(scene.s, &p_, &a_), "pt_adaptive_create");
  }
  ~accumulator() { pt_accum_destroy(a_); }
  accumulator(const accumulator&) = delete;
  accumulator& operator=(const accumulator&) = delete;

  // the next `samples` samples of every pixel
  void add(int samples, void* stream = nullptr) { check(pt_render_accumulate(a_, &cam_, samples, stream), "pt_render_accumulate"); }
  // adaptive: the next `samples` samples of the pixels whose mask byte is nonzero (nullptr: every pixel; a mask synchronises `stream`)
  void add_masked(int samples, const uint8_t* mask_device, void* stream = nullptr) {
    check(pt_adaptive_window(a_, &cam_, samples, mask_device, stream), "pt_adaptive_window");
  }
  void counts(int32_t* counts_device, void* stream = nullptr) const { check(pt_adaptive_counts(a_, counts_device, stream), "pt_adaptive_counts"); }
  void error(float* err_device, void* stream = nullptr) const { check(pt_adaptive_error(a_, err_device, stream), "pt_adaptive_error"); }
  // adaptive: the per-channel variance of each resolved pixel from the two half buffers (a DEVICE buffer of pt_framebuffer_floats()
  // floats, laid out like the frame) — what variance_denoise() takes
  void variance(float* variance_device, void* stream = nullptr) const { check(pt_variance_estimate(a_, variance_device, stream), "pt_variance_estimate"); }
  // the next window's mask; returns how many pixels are active (synchronises `stream`)
  int64_t select(float threshold, int min_spp, int max_spp, bool dilate, uint8_t* mask_device, void* stream = nullptr) const {
    int64_t n = 0;
    check(pt_adaptive_select(a_, threshold, min_spp, max_spp, dilate ? PT_ADAPTIVE_DILATE : 0u, mask_device, &n, stream), "pt_adaptive_select");
    return n;
  }
  bool is_adaptive() const { return adaptive_; }
  // adaptive: each pixel's count, from an exported state (host memory)
  std::vector<int32_t> counts() const {
    const std::vector<uint8_t> st = state();
    const std::size_t F = (std::size_t)pt_framebuffer_floats(&p_), R = (std::size_t)pt_shard_tiles(&p_) * PT_TILE_PIXELS;
    std::vector<int32_t> n(F / 3);
    std::memcpy(n.data(), st.data() + PT_ACCUM_HEADER_BYTES + 8 * F + 4 * R, n.size() * sizeof(int32_t));
    return n;
  }
  int samples() const { return pt_accum_samples(a_); }
  void reset(void* stream = nullptr) { check(pt_accum_reset(a_, stream), "pt_accum_reset"); }
  // adaptive: a new image that CONTINUES every pixel's random stream (pt_adaptive_next_frame) — the frames of a sequence then carry
  // independent noise, which is what pt::temporal averages; the next window binds `cam` (or the camera used so far)
  void next_frame(void* stream = nullptr) { check(pt_adaptive_next_frame(a_, stream), "pt_adaptive_next_frame"); }
  void next_frame(const camera& cam, void* stream = nullptr) {
    next_frame(stream);
    cam_ = cam.c;
  }

  // the mean so far, in render()'s layout (host memory: from the exported sums, divided here with the same correctly rounded IEEE
  // division as the device's resolve — the host build has no fast-math, no contraction)
  void resolve(frame_buffer& frame_buf) const {
    if (!adaptive_ && samples() <= 0) throw pt_error(PT_ERR_INVALID_ARG, "accumulator::resolve: no samples rendered yet");
    const std::vector<uint8_t> st = state();
    const std::size_t floats = (std::size_t)pt_framebuffer_floats(&p_);
    std::vector<int32_t> n;
    if (adaptive_) { // (refused before the first window, as pt_accum_resolve: no pixel has a sample yet)
      n = counts();
      if (std::all_of(n.begin(), n.end(), [](int32_t v) { return v == 0; }))
        throw pt_error(PT_ERR_INVALID_ARG, "accumulator::resolve: no samples rendered yet");
    }
    frame_buf.resize(floats / 3);
    static_assert(sizeof(color) == 12);
    float* out = reinterpret_cast<float*>(frame_buf.data());
    std::memcpy(out, st.data() + PT_ACCUM_HEADER_BYTES, floats * sizeof(float));
    if (adaptive_) { // each pixel by its own count (0 where it has none)
      for (std::size_t i = 0; i < floats; i++) out[i] = n[i / 3] > 0 ? out[i] / (float)n[i / 3] : 0.0f;
      return;
    }
    const float done = (float)samples();
    for (std::size_t i = 0; i < floats; i++) out[i] = out[i] / done;
  }

  // checkpoint (pt_accum_export's format) / restore into this accumulator (same frame parameters; the camera comes with the state)
  // (adaptive: pt_adaptive_export's format; restore() also takes a plain accumulator's state and continues it adaptively)
  std::vector<uint8_t> state() const {
    if (adaptive_) {
      std::vector<uint8_t> st((std::size_t)pt_adaptive_state_bytes(&p_));
      check(pt_adaptive_export(a_, st.data(), (int64_t)st.size(), nullptr), "pt_adaptive_export");
      return st;
    }
    std::vector<uint8_t> st((std::size_t)pt_accum_state_bytes(&p_));
    check(pt_accum_export(a_, st.data(), (int64_t)st.size(), nullptr), "pt_accum_export");
    return st;
  }
  void restore(const std::vector<uint8_t>& st) {
    if (adaptive_) check(pt_adaptive_import(a_, st.data(), (int64_t)st.size(), nullptr), "pt_adaptive_import");
    else check(pt_accum_import(a_, st.data(), (int64_t)st.size(), nullptr), "pt_accum_import");
    int32_t bound = 0;
    std::memcpy(&bound, st.data() + 36, sizeof bound); // the header's "camera bound" word
    if (bound) std::memcpy(&cam_, st.data() + PT_ACCUM_HEADER_BYTES - sizeof(PtCamera), sizeof(PtCamera));
  }
  void save(const std::string& path) const {
    const std::vector<uint8_t> st = state();
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(st.data(), 1, st.size(), f) != st.size()) { if (f) std::fclose(f); throw std::runtime_error("accumulator::save: cannot write " + path); }
    std::fclose(f);
  }
  // (adaptive: a plain accumulator's checkpoint too, continued adaptively)
  void load(const std::string& path) {
    const std::size_t plain = (std::size_t)pt_accum_state_bytes(&p_), full = adaptive_ ? (std::size_t)pt_adaptive_state_bytes(&p_) : plain;
    std::vector<uint8_t> st(full + 1);
    std::FILE* f = std::fopen(path.c_str(), "rb");
    const std::size_t got = f ? std::fread(st.data(), 1, st.size(), f) : 0;
    if (f) std::fclose(f);
    if (got != full && got != plain) throw std::runtime_error("accumulator::load: " + path + " is not a state of this accumulator's size");
    st.resize(got);
    restore(st);
  }
  PtAccum* handle() const { return a_; }

 private:
  PtCamera cam_;
  PtRenderParams p_;
  PtAccum* a_ = nullptr;
  bool adaptive_ = false;
};

} // namespace pt
