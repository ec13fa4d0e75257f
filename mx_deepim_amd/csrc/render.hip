// GPU rasteriser for the step BETWEEN refinement iterations: replaces the OpenGL off-screen
// render + glReadPixels of lib/render_glumpy/render_py_multi.py:101-129 so the render-and-compare loop never
// leaves the device. Same camera model: u0 = cx + 0.5 with GL pixel centres at +0.5 (:132-147) means a camera
// point projects to pixel-INDEX coordinates u = fx·X/Z + cx, v = fy·Y/Z + cy and a pixel is covered when its
// index (i, j) lies inside the projected triangle; depth test GL_LESS, no face culling, no blending (:93-95);
// depth read-back is linearised to metric z (:126-128) — here z is kept metric throughout; colour is the
// texture (GL_LINEAR, clamp) at perspective-correct uv, or perspective-correct vertex colours.
// OpenGL's exact rasterisation (sub-pixel snapping, 24-bit depth) cannot run here: PARITY UNPINNED, restated as
// standard top-left-rule rasterisation; the tests check it against a CPU restatement and an analytic ray cast.
//
// Three kernels, all per-pair batched, templated on where a sample's mesh comes from (OneMesh: the whole batch draws one
// mesh; MeshTable: every sample picks its mesh by a device-resident class id). The per-sample arithmetic is one text:
//   project:  one thread per (pair, vertex): camera transform + projection → (u, v, Z)
//   raster:   one thread per (pair, triangle): walks the triangle's clipped bounding box, interpolates 1/Z
//             (affine in screen space, like GL's z) and resolves visibility with ONE 64-bit atomicMin per
//             covered pixel on the key (float_bits(Z) << 32 | triangle id) — first triangle wins exact ties
//   resolve:  one thread per pixel: re-derives the barycentrics of the winning triangle, shades, writes the
//             network tensors directly: image (B,3,H,W) RGB mean-subtracted, depth (B,1,H,W), 0 = background
//             (resolve_frames_kernel: the same fragment with a light per sample, stored as uint8 / uint16 frames;
//             resolve_scene_kernel: several objects per frame in one z-buffer plane, the key carrying the object's slot)
#include "common.h"
#include <limits.h>

namespace {

struct PV { float u, v, z; };

// One mesh as the kernels see it. attr: per-vertex attributes — 3 floats RGB (0..255) when tex == nullptr, else 2 floats uv.
// normals != nullptr selects the lit fragment stage.
struct MeshRef {
  const float* verts;    // (V,3) model-space positions
  const float* attr;
  const float* normals;  // (V,3) or nullptr
  const int* faces;      // (F,3), indices local to this mesh
  const float* tex;      // (TH,TW,3) or nullptr
  int TH, TW, V, F;
};

// Mesh source of the single-mesh entries: every sample draws `m`; the projected-vertex scratch is B x V records.
struct OneMesh {
  MeshRef m;
  __device__ __forceinline__ bool mesh(int, MeshRef& o) const { o = m; return true; }
  __device__ __forceinline__ int pv_stride() const { return m.V; }
};

// Mesh source of deepim_render_classes_forward: sample b draws the mesh of class_index[b] out of back-to-back arrays described
// by rows {v_off, V, f_off, F, attr_off, tex_off, tex_h, tex_w} of `desc`. The id and the row depend on blockIdx.y only, so they
// are scalar loads. An id outside [0, n_classes) — or a textured row in a table without textures — selects no mesh: the sample
// stays an empty frame and nothing outside the table is read. V and F are clipped to the scratch's max_V / max_F records.
struct MeshTable {
  const int* class_index;
  const int* desc;
  const float* verts;
  const float* attr;
  const float* normals;
  const int* faces;
  const float* tex;
  int n_classes, max_V, max_F;
  __device__ __forceinline__ bool mesh(int b, MeshRef& o) const {
    const int cls = class_index[b];
    if ((unsigned)cls >= (unsigned)n_classes) return false;
    const int* d = desc + (long)cls * 8;
    const int v_off = d[0], f_off = d[2], attr_off = d[4], tex_off = d[5];
    if (tex_off >= 0 && tex == nullptr) return false;
    o.V = min(d[1], max_V); o.F = min(d[3], max_F);
    o.verts = verts + (long)v_off * 3;
    o.normals = normals != nullptr ? normals + (long)v_off * 3 : nullptr;
    o.faces = faces + (long)f_off * 3;
    o.attr = attr + attr_off;
    o.tex = tex_off >= 0 ? tex + tex_off : nullptr;
    o.TH = d[6]; o.TW = d[7];
    return true;
  }
  __device__ __forceinline__ int pv_stride() const { return max_V; }
};

// Cam: CamOne (K by value) or CamTable (sample b = blockIdx.y reads row b of the bound table: a uniform load). A non-finite row
// projects its sample to non-finite vertices, which the raster pass drops: an empty draw, and no address depends on the row.
template <class Src, class Cam>
__global__ __launch_bounds__(256) void project_kernel(PV* __restrict__ pv, Src src, const float* __restrict__ poses, Cam cam,
                                                      int* __restrict__ box_words) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  // arm this sample's bbox accumulator for the resolve pass of THIS call, in stream order (two launches earlier):
  // no state survives between calls, so changing B between calls or replaying a captured graph is safe
  if (box_words != nullptr && i < 4) box_words[b * 4 + i] = (i & 1) ? -1 : INT_MAX;
  MeshRef m;
  if (!src.mesh(b, m) || i >= m.V) return;
  const float* __restrict__ verts = m.verts;
  const float* P = poses + b * 12;
  const float x = verts[i * 3], y = verts[i * 3 + 1], z = verts[i * 3 + 2];
  const float X = ((P[0] * x + P[1] * y) + P[2] * z) + P[3];
  const float Y = ((P[4] * x + P[5] * y) + P[6] * z) + P[7];
  const float Z = ((P[8] * x + P[9] * y) + P[10] * z) + P[11];
  const auto& K = cam.at(b);
  PV o;
  o.u = K.v[0] * X / Z + K.v[2];
  o.v = K.v[4] * Y / Z + K.v[5];
  o.z = Z;
  pv[(long)b * src.pv_stride() + i] = o;
}

// edge function of pixel (px,py) against edge a→b; > 0 on the interior side for the orientation used below
__device__ __forceinline__ float edge_fn(float ax, float ay, float bx, float by, float px, float py) {
  return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}
// top-left rule (image coordinates, y down) for an edge with direction (dx,dy) of a triangle oriented so that edge_fn
// is positive inside: the top edge runs left→right, left edges run upwards
__device__ __forceinline__ bool top_left(float dx, float dy) { return (dy == 0.f && dx > 0.f) || dy < 0.f; }

struct Tri { float ax, ay, az, bx, by, bz, cx, cy, cz; bool ok; };

__device__ __forceinline__ Tri load_tri(const PV* __restrict__ pv, const int* __restrict__ faces, int f, float znear,
                                        int& ia, int& ib, int& ic) {
  ia = faces[f * 3]; ib = faces[f * 3 + 1]; ic = faces[f * 3 + 2];
  PV a = pv[ia], b = pv[ib], c = pv[ic];
  Tri t;
  t.ok = a.z > znear && b.z > znear && c.z > znear;  // triangles crossing the near plane are dropped, not clipped
  const float area = edge_fn(a.u, a.v, b.u, b.v, c.u, c.v);
  if (area == 0.f || !(area == area)) t.ok = false;
  if (area < 0.f) { PV tmp = b; b = c; c = tmp; const int ti = ib; ib = ic; ic = ti; }  // no culling: orient positively
  t.ax = a.u; t.ay = a.v; t.az = a.z; t.bx = b.u; t.by = b.v; t.bz = b.z; t.cx = c.u; t.cy = c.v; t.cz = c.z;
  return t;
}

// barycentric weights of pixel (x,y) (w0 ↔ a, w1 ↔ b, w2 ↔ c) and coverage under the top-left rule
__device__ __forceinline__ bool cover(const Tri& t, float x, float y, float& w0, float& w1, float& w2) {
  w0 = edge_fn(t.bx, t.by, t.cx, t.cy, x, y);
  w1 = edge_fn(t.cx, t.cy, t.ax, t.ay, x, y);
  w2 = edge_fn(t.ax, t.ay, t.bx, t.by, x, y);
  const bool i0 = w0 > 0.f || (w0 == 0.f && top_left(t.cx - t.bx, t.cy - t.by));
  const bool i1 = w1 > 0.f || (w1 == 0.f && top_left(t.ax - t.cx, t.ay - t.cy));
  const bool i2 = w2 > 0.f || (w2 == 0.f && top_left(t.bx - t.ax, t.by - t.ay));
  return i0 && i1 && i2;
}

__device__ __forceinline__ float pixel_depth(const Tri& t, float w0, float w1, float w2) {
  const float sum = (w0 + w1) + w2;
  const float inv = ((w0 / t.az + w1 / t.bz) + w2 / t.cz) / sum;  // 1/Z is affine in screen space
  return 1.0f / inv;
}

// Where a sample's fragments go. OwnPlane: sample b owns z-buffer plane b and its keys carry the triangle id alone.
// ScenePlane (deepim_render_scene_forward): sample d = f S + s is slot s of frame f; the S slots of a frame share plane f and a
// key carries the slot in bits 24..31 of its low word, above the triangle id (max_F <= 2^24), so that between objects the
// nearer fragment wins and an exact depth tie goes to the lower slot; within a slot the order is the single-object draw's.
struct OwnPlane {
  __device__ __forceinline__ int plane(int b) const { return b; }
  __device__ __forceinline__ unsigned tag(int) const { return 0u; }
};
struct ScenePlane {
  int S;
  __device__ __forceinline__ int plane(int d) const { return d / S; }
  __device__ __forceinline__ unsigned tag(int d) const { return (unsigned)(d % S) << 24; }
};

template <class Src, class Plane>
__global__ __launch_bounds__(256) void raster_kernel(unsigned long long* __restrict__ zbuf, const PV* __restrict__ pv_all,
                                                     Src src, Plane plane, int H, int W, float znear, float zfar) {
  const int b = blockIdx.y, f = blockIdx.x * 256 + threadIdx.x;
  MeshRef m;
  if (!src.mesh(b, m) || f >= m.F) return;
  int ia, ib, ic;
  const Tri t = load_tri(pv_all + (long)b * src.pv_stride(), m.faces, f, znear, ia, ib, ic);
  if (!t.ok) return;
  const float minx = fminf(t.ax, fminf(t.bx, t.cx)), maxx = fmaxf(t.ax, fmaxf(t.bx, t.cx));
  const float miny = fminf(t.ay, fminf(t.by, t.cy)), maxy = fmaxf(t.ay, fmaxf(t.by, t.cy));
  if (!(maxx >= 0.f && minx <= (float)(W - 1) && maxy >= 0.f && miny <= (float)(H - 1))) return;
  const int x0 = max(0, (int)ceilf(minx)), x1 = min(W - 1, (int)floorf(maxx));
  const int y0 = max(0, (int)ceilf(miny)), y1 = min(H - 1, (int)floorf(maxy));
  unsigned long long* zb = zbuf + (long)plane.plane(b) * H * W;
  const unsigned low = plane.tag(b) | (unsigned)f;
  for (int y = y0; y <= y1; ++y)
    for (int x = x0; x <= x1; ++x) {
      float w0, w1, w2;
      if (!cover(t, (float)x, (float)y, w0, w1, w2)) continue;
      const float z = pixel_depth(t, w0, w1, w2);
      if (!(z > znear && z < zfar)) continue;  // GL clips fragments outside [zNear, zFar]
      const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | low;
      atomicMin(zb + (long)y * W + x, key);
    }
}

__device__ __forceinline__ float tex_bilinear(const float* __restrict__ tex, int TH, int TW, int c, float u, float v) {
  // GL_LINEAR with clamp-to-edge; texel centres at (i + 0.5) / size; v = 0 is the FIRST row of `tex`
  const float x = u * TW - 0.5f, y = v * TH - 0.5f;
  const float xf = floorf(x), yf = floorf(y);
  const float fx = x - xf, fy = y - yf;
  const int x0 = min(max((int)xf, 0), TW - 1), x1 = min(max((int)xf + 1, 0), TW - 1);
  const int y0 = min(max((int)yf, 0), TH - 1), y1 = min(max((int)yf + 1, 0), TH - 1);
  const float t00 = tex[(y0 * TW + x0) * 3 + c], t01 = tex[(y0 * TW + x1) * 3 + c];
  const float t10 = tex[(y1 * TW + x0) * 3 + c], t11 = tex[(y1 * TW + x1) * 3 + c];
  const float top = t00 + (t01 - t00) * fx, bot = t10 + (t11 - t10) * fx;
  return top + (bot - top) * fy;
}

// Lit fragment stage of the ModelNet loop (lib/render_glumpy/render_py_light_modelnet_multi.py:36-80, light set-up
// deepim/core/tester.py:146-172 = batch_updater_py_multi.py:185-228). All of it in OpenGL camera coordinates (y, z flipped):
//   position = u_view·u_model·v_position,  normal = (u_view·u_model)^-T·(v_normal, 1) — whose 4-vector normalisation cancels in
//   the next line —  brightness = clamp(n·(L − position) / (|L − position|·|n|), 0, 1),
//   colour = texture·((1 − r) + r·brightness)·intensity, read back as round(clamp(colour, 0, 1)·255) (:162-166: uint8).
// L = light_offset + (t_x, −t_y, −t_z) of the sample's pose. v_position / v_normal are the mesh's verts / normals; a mesh without
// normals takes the unlit stage of render_py_multi.py.
struct LitParams {
  const float* poses;      // (B,3,4)
  const float* intensity;  // (B,3) device, or nullptr = (1,1,1)
  Vec3 light_offset;       // 0.5·(0,1,1) in the reference's loops
  float ratio;             // brightness_ratio (0.7)
  static constexpr bool lit = true;
  __device__ __forceinline__ float offset(int, int r) const { return light_offset.v[r]; }
  __device__ __forceinline__ float inten(int b, int c) const { return intensity ? intensity[b * 3 + c] : 1.f; }
  __device__ __forceinline__ float rat(int) const { return ratio; }
};

// Light source of deepim_render_observed_forward: every sample has its own light (LM6d_ds_1_gen_observed.py:116-144), three
// device arrays with one row per sample. b is blockIdx.y, so these are scalar loads.
struct LitPerSample {
  const float* poses;      // (B,3,4)
  const float* off;        // (B,3)
  const float* intensity;  // (B,3)
  const float* ratio;      // (B)
  static constexpr bool lit = true;
  __device__ __forceinline__ float offset(int b, int r) const { return off[b * 3 + r]; }
  __device__ __forceinline__ float inten(int b, int c) const { return intensity[b * 3 + c]; }
  __device__ __forceinline__ float rat(int b) const { return ratio[b]; }
  // the stored byte of a level: the lit stage's levels are whole numbers in 0..255 already
  static __device__ __forceinline__ unsigned level(float v) { return (unsigned)(int)v; }
};

// Light source of deepim_render_frames_forward: none. The lit stage is compiled out and a level is the unlit one (texture or
// vertex colour, any float), stored as cv2.imwrite converts a float image (toolkit/LM6d_3_gen_PoseCNN_pred_rendered.py:149-155): saturated,
// rounded to nearest even.
struct Unlit {
  static constexpr bool lit = false;
  static __device__ __forceinline__ unsigned level(float v) { return (unsigned)(int)rintf(fminf(fmaxf(v, 0.f), 255.f)); }
};

// The fragment of pixel p of sample b from its z-buffer key (hit = the key is not all-ones): depth z (0 = background) and colour
// levels rgb (the lit stage's are whole numbers in 0..255). One text for every resolve kernel, whatever it stores (tensors or
// frames) and wherever its light comes from (Lit: LitParams or LitPerSample).
struct Frag { float rgb[3]; float z; };
template <class Src, class Lit>
__device__ __forceinline__ Frag resolve_pixel(bool hit, unsigned long long key, int b, long p, const PV* pv_all,
                                               const Src& src, int W, float znear, const Lit& lit) {
  float rgb[3] = {0.f, 0.f, 0.f};
  float z = 0.f;
  MeshRef m;
  if (hit && src.mesh(b, m)) {      // only a sample with a mesh ever rasterised a key
    const float* __restrict__ attr = m.attr;
    const float* __restrict__ tex = m.tex;
    const int f = (int)(unsigned)(key & 0xffffffffu);
    z = __uint_as_float((unsigned)(key >> 32));
    int ia, ib, ic;
    const Tri t = load_tri(pv_all + (long)b * src.pv_stride(), m.faces, f, znear, ia, ib, ic);
    const int y = (int)(p / W), x = (int)(p - (long)y * W);
    float w0, w1, w2;
    cover(t, (float)x, (float)y, w0, w1, w2);
    // perspective-correct weights
    const float q0 = w0 / t.az, q1 = w1 / t.bz, q2 = w2 / t.cz;
    const float qs = (q0 + q1) + q2;
    if (tex == nullptr) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        rgb[c] = ((q0 * attr[ia * 3 + c] + q1 * attr[ib * 3 + c]) + q2 * attr[ic * 3 + c]) / qs;
    } else {
      const float u = ((q0 * attr[ia * 2] + q1 * attr[ib * 2]) + q2 * attr[ic * 2]) / qs;
      const float v = ((q0 * attr[ia * 2 + 1] + q1 * attr[ib * 2 + 1]) + q2 * attr[ic * 2 + 1]) / qs;
#pragma unroll
      for (int c = 0; c < 3; ++c) rgb[c] = tex_bilinear(tex, m.TH, m.TW, c, u, v);
    }
    if constexpr (Lit::lit) if (m.normals != nullptr) {
      const float* P = lit.poses + b * 12;
      float mp[3], mn[3];      // perspective-correct model-space position and normal of the fragment (GL varyings)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        mp[c] = ((q0 * m.verts[ia * 3 + c] + q1 * m.verts[ib * 3 + c]) + q2 * m.verts[ic * 3 + c]) / qs;
        mn[c] = ((q0 * m.normals[ia * 3 + c] + q1 * m.normals[ib * 3 + c]) + q2 * m.normals[ic * 3 + c]) / qs;
      }
      float pos[3], nrm[3], s2l[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const float sgn = r == 0 ? 1.f : -1.f;     // yz_flip of _get_view_mtx
        pos[r] = sgn * ((((P[r * 4] * mp[0] + P[r * 4 + 1] * mp[1]) + P[r * 4 + 2] * mp[2])) + P[r * 4 + 3]);
        nrm[r] = sgn * ((P[r * 4] * mn[0] + P[r * 4 + 1] * mn[1]) + P[r * 4 + 2] * mn[2]);
        s2l[r] = (lit.offset(b, r) + sgn * P[r * 4 + 3]) - pos[r];
      }
      const float dotp = (nrm[0] * s2l[0] + nrm[1] * s2l[1]) + nrm[2] * s2l[2];
      const float ls = sqrtf((s2l[0] * s2l[0] + s2l[1] * s2l[1]) + s2l[2] * s2l[2]);
      const float ln = sqrtf((nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2]);
      float br = dotp / (ls * ln);
      br = fmaxf(fminf(br, 1.f), 0.f);             // max(min(x, 1), 0): a NaN (degenerate normal) becomes 0, as in GLSL on most drivers
      if (!(br == br)) br = 0.f;
      const float ratio = lit.rat(b);
      const float shade = (1.f - ratio) + ratio * br;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float inten = lit.inten(b, c);
        float col = (rgb[c] / 255.f) * (shade * inten);
        col = fminf(fmaxf(col, 0.f), 1.f);
        rgb[c] = rintf(col * 255.f);               // np.round(rgb * 255).astype(uint8)
      }
    }
  }
  Frag o;
  o.rgb[0] = rgb[0]; o.rgb[1] = rgb[1]; o.rgb[2] = rgb[2]; o.z = z;
  return o;
}

// The lane's PX consecutive z-buffer keys (PX = 4 or 1), put back to all-ones where an object was: the z-buffer leaves the call
// as it entered it. With PX = 4 the keys are 32 contiguous, 32-byte aligned bytes: two 16-byte loads.
template <int PX>
__device__ __forceinline__ void take_keys(unsigned long long* zb, unsigned long long (&keys)[PX]) {
  if constexpr (PX == 4) {
    const ulonglong2 k01 = reinterpret_cast<const ulonglong2*>(zb)[0], k23 = reinterpret_cast<const ulonglong2*>(zb)[1];
    keys[0] = k01.x; keys[1] = k01.y; keys[2] = k23.x; keys[3] = k23.y;
    if ((k01.x & k01.y & k23.x & k23.y) != ~0ull) {
      const ulonglong2 ones = {~0ull, ~0ull};
      reinterpret_cast<ulonglong2*>(zb)[0] = ones;
      reinterpret_cast<ulonglong2*>(zb)[1] = ones;
    }
  } else {
    keys[0] = zb[0];
    if (keys[0] != ~0ull) zb[0] = ~0ull;
  }
}

// One value per owned pixel of one output plane: PX = 4 as one 16-byte store.
template <int PX>
__device__ __forceinline__ void store_plane_pixels(float* dst, const float (&v)[PX]) {
  if constexpr (PX == 4) *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
  else dst[0] = v[0];
}

// Resolve pass of the tensor entries: lane g of a sample owns the PX consecutive pixels PX g .. PX g + PX - 1. PX = 4 (the plane
// is a multiple of 4 pixels and every output is 16-byte aligned): the keys come as two 16-byte loads and each output plane takes
// one 16-byte store per lane; PX = 1: any size. Both give every pixel the same fragment and the box words the same reduction.
// No lane leaves early: the box reduction shuffles across the whole wave.
template <class Src, int PX>
__global__ __launch_bounds__(256) void resolve_kernel(float* __restrict__ image, float* __restrict__ depth,
                                                      unsigned long long* __restrict__ zbuf,
                                                      const PV* __restrict__ pv_all, Src src, Vec3 means, int H, int W,
                                                      float znear, float* __restrict__ mask, float mask_thresh,
                                                      int* __restrict__ box_words, LitParams lit) {
  const int b = blockIdx.y;
  const long p = ((long)blockIdx.x * 256 + threadIdx.x) * PX;
  const long plane = (long)H * W;
  const bool inside = p < plane;                 // PX = 4: plane % 4 == 0, so a lane owns four pixels or none
  unsigned long long keys[PX];
#pragma unroll
  for (int i = 0; i < PX; ++i) keys[i] = ~0ull;
  if (inside) take_keys<PX>(zbuf + (long)b * plane + p, keys);
  float ch[3][PX], z[PX];
#pragma unroll
  for (int i = 0; i < PX; ++i) {
    const Frag fr = resolve_pixel(keys[i] != ~0ull, keys[i], b, p + i, pv_all, src, W, znear, lit);
#pragma unroll
    for (int c = 0; c < 3; ++c) ch[c][i] = fr.rgb[c] - means.v[c];
    z[i] = fr.z;
  }
  if (inside) {
#pragma unroll
    for (int c = 0; c < 3; ++c) store_plane_pixels<PX>(image + ((long)b * 3 + c) * plane + p, ch[c]);
    store_plane_pixels<PX>(depth + (long)b * plane + p, z);
  }
  if (mask != nullptr) {
    // fused tester.py:440-442 (mask_rendered = depth > thresh) and the bbox pass of the box_rendered rectangle
    float mk[PX];
    bool on = false;
    int xmin = INT_MAX, xmax = -1, ymin = INT_MAX, ymax = -1;
#pragma unroll
    for (int i = 0; i < PX; ++i) {
      const bool on_i = inside && z[i] > mask_thresh;
      mk[i] = on_i ? 1.f : 0.f;
      if (on_i) {
        const int y = (int)((p + i) / W), x = (int)(p + i - (long)y * W);
        xmin = min(xmin, x); xmax = max(xmax, x); ymin = min(ymin, y); ymax = max(ymax, y);
      }
      on = on || on_i;
    }
    if (inside) store_plane_pixels<PX>(mask + (long)b * plane + p, mk);
    if (box_words != nullptr && __ballot(on) != 0ull) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        xmin = min(xmin, __shfl_xor(xmin, off, 64)); xmax = max(xmax, __shfl_xor(xmax, off, 64));
        ymin = min(ymin, __shfl_xor(ymin, off, 64)); ymax = max(ymax, __shfl_xor(ymax, off, 64));
      }
      if ((threadIdx.x & 63) == 0) {
        atomicMin(&box_words[b * 4 + 0], xmin); atomicMax(&box_words[b * 4 + 1], xmax);
        atomicMin(&box_words[b * 4 + 2], ymin); atomicMax(&box_words[b * 4 + 3], ymax);
      }
    }
  }
}

// Destination of deepim_render_observed_forward / deepim_render_frames_forward: decoded frames as lib/utils/image.py reads them
// from the PNGs of LM6d_ds_1_gen_observed.py:149-159, sample b in row rows[b] (nullptr: b) of N rows. 6 bytes per pixel.
struct FrameOut {
  unsigned char* image;         // (N,H,W,3) BGR levels
  unsigned short* depth;        // (N,H,W) (uint16)(depth * depth_factor), the float32 product truncated
  unsigned char* label;         // (N,H,W) label_value[b] where depth != 0, else 0; nullptr: not stored
  int* covered;                 // (B) zeroed before the launch: += the sample's pixels with a non-zero stored depth; or nullptr
  const int* rows;              // (B) or nullptr
  const int* label_value;       // (B) or nullptr = 1
  float depth_factor;
  int N;
};

// The far end of a frame resolve pass, for the PX consecutive pixels a lane owns (PX = 4 or 1); the near end is take_keys above.
// store_frame_pixels: BGR levels, uint16 depths and labels (label == nullptr: not stored) at pixel q of the (N,H,W[,3]) outputs.
template <int PX>
__device__ __forceinline__ void store_frame_pixels(unsigned char* image, unsigned short* depth, unsigned char* label, long q,
                                                   const unsigned (&bgr)[PX * 3], const unsigned (&d16)[PX], const unsigned (&l8)[PX]) {
  if constexpr (PX == 4) {
    uint3 w;
    w.x = bgr[0] | bgr[1] << 8 | bgr[2] << 16 | bgr[3] << 24;
    w.y = bgr[4] | bgr[5] << 8 | bgr[6] << 16 | bgr[7] << 24;
    w.z = bgr[8] | bgr[9] << 8 | bgr[10] << 16 | bgr[11] << 24;
    unsigned* img = reinterpret_cast<unsigned*>(image + q * 3);
    img[0] = w.x; img[1] = w.y; img[2] = w.z;
    uint2 d;
    d.x = d16[0] | d16[1] << 16;
    d.y = d16[2] | d16[3] << 16;
    *reinterpret_cast<uint2*>(depth + q) = d;
    if (label != nullptr) *reinterpret_cast<unsigned*>(label + q) = l8[0] | l8[1] << 8 | l8[2] << 16 | l8[3] << 24;
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) image[q * 3 + c] = (unsigned char)bgr[c];
    depth[q] = (unsigned short)d16[0];
    if (label != nullptr) label[q] = (unsigned char)l8[0];
  }
}

// Resolve pass of the frame draw: lane g of a sample owns the PX consecutive pixels PX g .. PX g + PX - 1.
// PX = 4 (the plane is a multiple of 4 pixels and the three outputs are 8-byte aligned): the lane stores its 12 image bytes as
// three dwords, its four depths as one 8-byte store and its four labels as one dword, so a wave writes 768 + 512 + 256
// contiguous bytes with no partial dwords. PX = 1: single byte / short stores, any size. A sample whose row is outside [0, N)
// stores nothing; its z-buffer entries are still put back and its pixels still counted. Lit: LitPerSample or Unlit, which also
// says how a level becomes a byte. The lanes past the plane are the tail of the grid's last waves, so lane 0 of a wave with any
// live lane is live: it adds the wave's count (ballots over the live lanes) to out.covered[b] with one atomic.
template <class Src, int PX, class Lit>
__global__ __launch_bounds__(256) void resolve_frames_kernel(FrameOut out, unsigned long long* __restrict__ zbuf,
                                                             const PV* __restrict__ pv_all, Src src, int H, int W, float znear,
                                                             Lit lit) {
  const int b = blockIdx.y;
  const long plane = (long)H * W;
  const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * PX;
  if (p0 >= plane) return;                       // PX = 4: plane % 4 == 0, so a lane owns four pixels or none
  const int row = out.rows ? out.rows[b] : b;
  const bool store = (unsigned)row < (unsigned)out.N;
  const unsigned lab = (unsigned)(out.label_value ? out.label_value[b] : 1) & 0xffu;
  unsigned long long* zb = zbuf + (long)b * plane + p0;
  unsigned bgr[PX * 3], d16[PX], l8[PX];
  unsigned long long keys[PX];
  take_keys<PX>(zb, keys);
#pragma unroll
  for (int i = 0; i < PX; ++i) {
    const unsigned long long key = keys[i];
    const bool hit = key != ~0ull;
    const Frag fr = resolve_pixel(hit, key, b, p0 + i, pv_all, src, W, znear, lit);
    const float* rgb = fr.rgb; const float z = fr.z;
#pragma unroll
    for (int c = 0; c < 3; ++c) bgr[i * 3 + c] = Lit::level(rgb[2 - c]);
    d16[i] = (unsigned)(int)(z * out.depth_factor) & 0xffffu;
    l8[i] = z != 0.f ? lab : 0u;
  }
  if (out.covered != nullptr) {
    int n = 0;
#pragma unroll
    for (int i = 0; i < PX; ++i) n += __popcll(__ballot(d16[i] != 0u));
    if (n != 0 && (threadIdx.x & 63) == 0) atomicAdd(out.covered + b, n);
  }
  if (!store) return;
  const long q = (long)row * plane + p0;
  store_frame_pixels<PX>(out.image, out.depth, out.label, q, bgr, d16, l8);
}

// Light source of deepim_render_scene_forward: one light per FRAME (render_py_light_multi_program.py:370-396 lights the objects of
// a scene with one light moved to each object's own pose), three device arrays with one row per frame. f is blockIdx.y, so these
// stay scalar loads; the pose is the slot's own, row d = f S + s of `poses`, and varies per lane.
struct LitPerFrame {
  const float* poses;      // (B S,3,4)
  const float* off;        // (B,3)
  const float* intensity;  // (B,3)
  const float* ratio;      // (B)
  int f;                   // set by the kernel: its frame
  static constexpr bool lit = true;
  __device__ __forceinline__ float offset(int, int r) const { return off[f * 3 + r]; }
  __device__ __forceinline__ float inten(int, int c) const { return intensity[f * 3 + c]; }
  __device__ __forceinline__ float rat(int) const { return ratio[f]; }
  static __device__ __forceinline__ unsigned level(float v) { return (unsigned)(int)v; }
};

// Destination of deepim_render_scene_forward: FrameOut's rows of decoded frames, one per frame f of S slots.
struct SceneOut {
  unsigned char* image;         // (N,H,W,3) BGR levels
  unsigned short* depth;        // (N,H,W)
  unsigned char* label;         // (N,H,W) label_value[f S + s] of the winning slot s where depth != 0, else 0
  int* visible;                 // (B,S) zeroed before the launch: += slot s's pixels of frame f with a non-zero stored depth; or nullptr
  const int* rows;              // (B) or nullptr
  const int* label_value;       // (B S) or nullptr = s + 1
  float depth_factor;
  int N, S;
};

// Resolve pass of the scene draw: resolve_frames_kernel over the B frames, each pixel shaded as the slot that won it. The slot
// sits in bits 24..31 of the key's low word (ScenePlane); it is taken out and the remaining key is what the single-object draw of
// sample f S + s leaves, so resolve_pixel gives that draw's fragment. The mesh row, the pose and the label value belong to the
// pixel's slot: they vary per lane inside a block and are vector loads here, no longer the scalar loads of the one-object
// passes; the light and the destination row depend on blockIdx.y alone and stay scalar. HBM-bound like its pattern: 8 B/px of
// key read (plus the put-back where an object was), 6 B/px stored. out.visible: per slot one ballot per owned pixel and at most
// one atomic add per wave, by lane 0 (live in every wave with a live lane, as in resolve_frames_kernel).
template <int PX>
__global__ __launch_bounds__(256) void resolve_scene_kernel(SceneOut out, unsigned long long* __restrict__ zbuf,
                                                            const PV* __restrict__ pv_all, MeshTable src, int H, int W, float znear,
                                                            LitPerFrame lit) {
  const int f = blockIdx.y, S = out.S;
  lit.f = f;
  const long plane = (long)H * W;
  const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * PX;
  if (p0 >= plane) return;                       // PX = 4: plane % 4 == 0, so a lane owns four pixels or none
  const int row = out.rows ? out.rows[f] : f;
  const bool store = (unsigned)row < (unsigned)out.N;
  unsigned long long* zb = zbuf + (long)f * plane + p0;
  unsigned bgr[PX * 3], d16[PX], l8[PX], slot[PX];
  unsigned long long keys[PX];
  take_keys<PX>(zb, keys);
#pragma unroll
  for (int i = 0; i < PX; ++i) {
    const unsigned s = (unsigned)(keys[i] >> 24) & 0xffu;
    const bool hit = keys[i] != ~0ull && s < (unsigned)S;      // the S slots' raster threads wrote every key: s < S; checked, since s makes addresses
    const unsigned long long key = keys[i] & ~0xff000000ull;
    const int d = f * S + (int)s;
    const Frag fr = resolve_pixel(hit, key, d, p0 + i, pv_all, src, W, znear, lit);
    const float* rgb = fr.rgb; const float z = fr.z;
#pragma unroll
    for (int c = 0; c < 3; ++c) bgr[i * 3 + c] = LitPerFrame::level(rgb[2 - c]);
    d16[i] = (unsigned)(int)(z * out.depth_factor) & 0xffffu;
    const unsigned lab = (unsigned)(out.label_value ? (hit ? out.label_value[d] : 0) : (int)s + 1) & 0xffu;
    l8[i] = z != 0.f ? lab : 0u;
    slot[i] = s;
  }
  if (out.visible != nullptr) {
    for (int s = 0; s < S; ++s) {
      int n = 0;
#pragma unroll
      for (int i = 0; i < PX; ++i) n += __popcll(__ballot(d16[i] != 0u && slot[i] == (unsigned)s));
      if (n != 0 && (threadIdx.x & 63) == 0) atomicAdd(out.visible + f * S + s, n);
    }
  }
  if (!store) return;
  const long q = (long)row * plane + p0;
  store_frame_pixels<PX>(out.image, out.depth, out.label, q, bgr, d16, l8);
}

}  // namespace

// The front of every entry's launch group: project (grid (ceil(max_V/256), B)) and raster (grid (ceil(max_F/256), B)) into the
// context's z-buffer, which is left dirty: the caller launches a resolve pass next and clears ctx->zbuf_dirty.
// max_V / max_F: the largest mesh `src` can select; the projected-vertex scratch (*pv_out) is B x max_V records.
// plane: where the B samples' fragments go (OwnPlane: `planes` = B; ScenePlane{S}: `planes` = B / S frames).
template <class Src, class Plane>
static int render_front(deepim_ctx* ctx, const Src& src, const Plane& plane, int planes, int max_V, int max_F, const float* poses,
                        const float* K_host, int B, int H, int W, float znear, float zfar, int* words, PV** pv_out) {
  DI_REQUIRE(znear > 0.f && zfar > znear, "render: need 0 < zNear < zFar");
  const size_t zbytes = (size_t)planes * H * W * sizeof(unsigned long long);
  const size_t pbytes = (size_t)B * max_V * sizeof(PV);
  void* scratch;
  int rc = deepim_scratch(ctx, pbytes + 64, &scratch);
  if (rc) return rc;
  // The z-buffer is the context's own (not the shared scratch): all-ones between calls — the resolve pass resets what the raster
  // pass touched — so a draw carries no clearing pass (8 B/px of writes and one launch per refinement iteration). Grow-only.
  if (ctx->zbuf_bytes < zbytes) {
    DI_REQUIRE(!ctx->capturing, "render: z-buffer growth during graph capture; run the sequence once eagerly first");
    DI_CHECK(hipStreamSynchronize(ctx->stream));
    if (ctx->zbuf) DI_CHECK(hipFree(ctx->zbuf));
    ctx->zbuf = nullptr; ctx->zbuf_bytes = 0;
    DI_CHECK(hipMalloc((void**)&ctx->zbuf, zbytes));
    ctx->zbuf_bytes = zbytes;
    DI_CHECK(hipMemsetAsync(ctx->zbuf, 0xff, zbytes, ctx->stream));
    ctx->zbuf_dirty = 0;
  }
  if (ctx->zbuf_dirty) {      // an earlier draw rasterised but its resolve pass was never launched: stale depth keys
    DI_CHECK(hipMemsetAsync(ctx->zbuf, 0xff, ctx->zbuf_bytes, ctx->stream));
    ctx->zbuf_dirty = 0;
  }
  PV* pv = (PV*)scratch;
  if (K_host)
    hipLaunchKernelGGL((project_kernel<Src, CamOne>), dim3(di_div_up(max_V, 256), B), dim3(256), 0, ctx->stream, pv, src, poses,
                       cam_one(K_host), words);
  else      // the bound camera table (the entry has checked it with DI_CAMERA)
    hipLaunchKernelGGL((project_kernel<Src, CamTable>), dim3(di_div_up(max_V, 256), B), dim3(256), 0, ctx->stream, pv, src, poses,
                       CamTable{ctx->cam_table}, words);
  DI_LAUNCH_CHECK();
  ctx->zbuf_dirty = 1;
  hipLaunchKernelGGL((raster_kernel<Src, Plane>), dim3(di_div_up(max_F, 256), B), dim3(256), 0, ctx->stream, ctx->zbuf, pv, src, plane,
                     H, W, znear, zfar);
  *pv_out = pv;
  return 0;
}

// The launch group of the tensor entries: the front, resolve, box fill.
// One-shot request of deepim_render_export_boxes: every render entry takes it first, before anything can fail, so that it
// never outlives the call it was made for.
static int* take_export(deepim_ctx* ctx) {
  int* boxes = ctx->export_boxes;
  ctx->export_boxes = nullptr;
  return boxes;
}
#define DI_NO_EXPORT(ctx) \
  DI_REQUIRE(take_export(ctx) == nullptr, "render: a boxes export is armed (deepim_render_export_boxes), but this entry draws no mask_box")

template <class Src>
static int render_launch(deepim_ctx* ctx, float* image, float* depth, float* mask, float* mask_box, int* export_boxes,
                         float mask_thresh, const Src& src, int max_V, int max_F, const float* poses, const float* K_host,
                         const float* pixel_means_host, int B, int H, int W, float znear, float zfar,
                         const float* light_offset_host, const float* light_intensity, float ratio) {
  DI_REQUIRE(mask_box == nullptr || (mask != nullptr && B <= DI_MAX_BOX_SAMPLES), "render: mask_box needs mask, B <= 4096");
  DI_REQUIRE(export_boxes == nullptr || mask_box != nullptr, "render: the boxes export needs mask_box");
  Vec3 means = {{0, 0, 0}};
  if (pixel_means_host) for (int i = 0; i < 3; ++i) means.v[i] = pixel_means_host[i];
  int* words = mask_box ? ctx->box_words : nullptr;
  LitParams lit = {poses, light_intensity, {{0, 0, 0}}, ratio};
  if (light_offset_host) for (int i = 0; i < 3; ++i) lit.light_offset.v[i] = light_offset_host[i];
  PV* pv;
  int rc = render_front(ctx, src, OwnPlane{}, B, max_V, max_F, poses, K_host, B, H, W, znear, zfar, words, &pv);
  if (rc) return rc;
  unsigned long long* zbuf = ctx->zbuf;
  const long plane = (long)H * W;
  const bool quad = ctx->render_quad && plane % 4 == 0 && (((uintptr_t)image | (uintptr_t)depth | (uintptr_t)mask) & 15) == 0;
  if (quad)
    hipLaunchKernelGGL((resolve_kernel<Src, 4>), dim3(di_div_up(plane / 4, 256), B), dim3(256), 0, ctx->stream, image, depth, zbuf,
                       pv, src, means, H, W, znear, mask, mask_thresh, words, lit);
  else
    hipLaunchKernelGGL((resolve_kernel<Src, 1>), dim3(di_div_up(plane, 256), B), dim3(256), 0, ctx->stream, image, depth, zbuf,
                       pv, src, means, H, W, znear, mask, mask_thresh, words, lit);
  DI_LAUNCH_CHECK();
  ctx->zbuf_dirty = 0;        // the resolve pass is queued behind the raster pass: the buffer will be all-ones again
  if (mask_box) return deepim_mask_box_fill(ctx, mask_box, words, export_boxes, B, H, W);
  return 0;
}

static int render_impl(deepim_ctx* ctx, float* image, float* depth, float* mask, float* mask_box, int* export_boxes,
                       float mask_thresh, const float* vertices, const float* vertex_attr, const int32_t* faces, const float* texture,
                       int tex_h, int tex_w, const float* poses, const float* K_host, const float* pixel_means_host,
                       int V, int F, int B, int H, int W, float znear, float zfar, const float* normals = nullptr,
                       const float* light_offset_host = nullptr, const float* light_intensity = nullptr, float ratio = 0.f) {
  if (B == 0) return 0;
  DI_REQUIRE(V > 0 && F > 0 && H > 0 && W > 0, "render: empty mesh or image");
  const OneMesh src = {{vertices, vertex_attr, normals, (const int*)faces, texture, tex_h, tex_w, V, F}};
  return render_launch(ctx, image, depth, mask, mask_box, export_boxes, mask_thresh, src, V, F, poses, K_host, pixel_means_host, B, H, W, znear,
                       zfar, normals != nullptr ? light_offset_host : nullptr, light_intensity, ratio);
}

extern "C" int deepim_render_forward(deepim_ctx* ctx, float* image, float* depth, const float* vertices,
                                     const float* vertex_attr, const int32_t* faces, const float* texture,
                                     int tex_h, int tex_w, const float* poses, const float* K_host,
                                     const float* pixel_means_host, int V, int F, int B, int H, int W, float znear,
                                     float zfar) {
  DI_NO_EXPORT(ctx);
  DI_DEVICE(ctx);
  DI_CAMERA(ctx, K_host, B, "deepim_render_forward");
  return render_impl(ctx, image, depth, nullptr, nullptr, nullptr, 0.f, vertices, vertex_attr, faces, texture, tex_h, tex_w, poses,
                     K_host, pixel_means_host, V, F, B, H, W, znear, zfar);
}

extern "C" int deepim_render_update_forward(deepim_ctx* ctx, float* image, float* depth, float* mask_rendered,
                                            float* mask_box, float mask_thresh, const float* vertices,
                                            const float* vertex_attr, const int32_t* faces, const float* texture,
                                            int tex_h, int tex_w, const float* poses, const float* K_host,
                                            const float* pixel_means_host, int V, int F, int B, int H, int W,
                                            float znear, float zfar) {
  int* export_boxes = take_export(ctx);
  DI_DEVICE(ctx);
  DI_CAMERA(ctx, K_host, B, "deepim_render_update_forward");
  DI_REQUIRE(mask_rendered != nullptr, "render_update: mask_rendered is NULL");
  return render_impl(ctx, image, depth, mask_rendered, mask_box, export_boxes, mask_thresh, vertices, vertex_attr, faces, texture, tex_h,
                     tex_w, poses, K_host, pixel_means_host, V, F, B, H, W, znear, zfar);
}

// The same passes with the lit fragment stage of the ModelNet render machine (render_py_light_modelnet_multi.py:36-80,170-188;
// the render closures of tester.py:146-184 and batch_updater_py_multi.py:185-228): see LitParams above.
extern "C" int deepim_render_lit_forward(deepim_ctx* ctx, float* image, float* depth, float* mask_rendered, float* mask_box,
                                         float mask_thresh, const float* vertices, const float* vertex_attr,
                                         const float* normals, const int32_t* faces, const float* texture, int tex_h,
                                         int tex_w, const float* poses, const float* K_host, const float* pixel_means_host,
                                         const float* light_offset_host, const float* light_intensity,
                                         float brightness_ratio, int V, int F, int B, int H, int W, float znear, float zfar) {
  int* export_boxes = take_export(ctx);
  DI_DEVICE(ctx);
  DI_CAMERA(ctx, K_host, B, "deepim_render_lit_forward");
  DI_REQUIRE(normals != nullptr && light_offset_host != nullptr, "render_lit: normals and light offset are required");
  DI_REQUIRE(brightness_ratio >= 0.f && brightness_ratio <= 1.f, "render_lit: brightness_ratio in [0, 1]");
  DI_REQUIRE(mask_box == nullptr || mask_rendered != nullptr, "render_lit: mask_box needs mask_rendered");
  return render_impl(ctx, image, depth, mask_rendered, mask_box, export_boxes, mask_thresh, vertices, vertex_attr, faces, texture,
                     tex_h, tex_w, poses, K_host, pixel_means_host, V, F, B, H, W, znear, zfar, normals, light_offset_host, light_intensity,
                     brightness_ratio);
}

// One launch group for a batch whose samples belong to different meshes: sample b draws class class_index[b] of the mesh table
// (layout: include/deepim_hip.h). normals == NULL: the unlit draw; else the lit one. The host never sees the ids.
extern "C" int deepim_render_classes_forward(deepim_ctx* ctx, float* image, float* depth, float* mask_rendered, float* mask_box,
                                             float mask_thresh, const int32_t* class_index, const int32_t* mesh_desc,
                                             int n_classes, int max_V, int max_F, const float* vertices,
                                             const float* vertex_attr, const float* normals, const int32_t* faces,
                                             const float* textures, const float* poses, const float* K_host,
                                             const float* pixel_means_host, const float* light_offset_host,
                                             const float* light_intensity, float brightness_ratio, int B, int H, int W,
                                             float znear, float zfar) {
  int* export_boxes = take_export(ctx);
  DI_DEVICE(ctx);
  if (B == 0) return 0;
  DI_CAMERA(ctx, K_host, B, "deepim_render_classes_forward");
  DI_REQUIRE(n_classes > 0 && max_V > 0 && max_F > 0 && H > 0 && W > 0, "render_classes: empty mesh table or image");
  DI_REQUIRE(class_index != nullptr && mesh_desc != nullptr, "render_classes: class_index and mesh_desc are required");
  DI_REQUIRE(mask_box == nullptr || mask_rendered != nullptr, "render_classes: mask_box needs mask_rendered");
  if (normals != nullptr) {
    DI_REQUIRE(light_offset_host != nullptr, "render_classes: the lit draw needs the light offset");
    DI_REQUIRE(brightness_ratio >= 0.f && brightness_ratio <= 1.f, "render_classes: brightness_ratio in [0, 1]");
  } else {
    DI_REQUIRE(light_offset_host == nullptr && light_intensity == nullptr, "render_classes: the lit draw needs normals");
  }
  const MeshTable src = {(const int*)class_index, (const int*)mesh_desc, vertices, vertex_attr, normals, (const int*)faces,
                         textures, n_classes, max_V, max_F};
  return render_launch(ctx, image, depth, mask_rendered, mask_box, export_boxes, mask_thresh, src, max_V, max_F, poses, K_host,
                       pixel_means_host, B, H, W, znear, zfar, light_offset_host, light_intensity, brightness_ratio);
}

// The launch group of the frame entries: the front, then the frame resolve pass with the light source `lit`.
template <class Lit>
static int frames_launch(deepim_ctx* ctx, const FrameOut& out, const MeshTable& src, const Lit& lit, int max_V, int max_F,
                         const float* poses, const float* K_host, int B, int H, int W, float znear, float zfar) {
  PV* pv;
  int rc = render_front(ctx, src, OwnPlane{}, B, max_V, max_F, poses, K_host, B, H, W, znear, zfar, nullptr, &pv);
  if (rc) return rc;
  const long plane = (long)H * W;
  const bool quad = plane % 4 == 0 && (((uintptr_t)out.image | (uintptr_t)out.depth | (uintptr_t)out.label) & 7) == 0;
  if (quad)
    hipLaunchKernelGGL((resolve_frames_kernel<MeshTable, 4, Lit>), dim3(di_div_up(plane / 4, 256), B), dim3(256), 0, ctx->stream,
                       out, ctx->zbuf, pv, src, H, W, znear, lit);
  else
    hipLaunchKernelGGL((resolve_frames_kernel<MeshTable, 1, Lit>), dim3(di_div_up(plane, 256), B), dim3(256), 0, ctx->stream, out,
                       ctx->zbuf, pv, src, H, W, znear, lit);
  DI_LAUNCH_CHECK();
  ctx->zbuf_dirty = 0;
  return 0;
}

// The mesh-table draw, lit, with one light per sample, written as decoded frames (layout: include/deepim_hip.h).
extern "C" int deepim_render_observed_forward(deepim_ctx* ctx, uint8_t* image, uint16_t* depth, uint8_t* label, const int32_t* rows,
                                              int N, const int32_t* label_value, float depth_factor, const int32_t* class_index,
                                              const int32_t* mesh_desc, int n_classes, int max_V, int max_F, const float* vertices,
                                              const float* vertex_attr, const float* normals, const int32_t* faces,
                                              const float* textures, const float* poses, const float* K_host,
                                              const float* light_offset, const float* light_intensity,
                                              const float* brightness_ratio, int B, int H, int W, float znear, float zfar) {
  DI_NO_EXPORT(ctx);
  DI_DEVICE(ctx);
  DI_REQUIRE(B >= 0 && N >= B, "render_observed: the outputs need N >= B >= 0 rows");
  if (B == 0) return 0;
  DI_CAMERA(ctx, K_host, B, "deepim_render_observed_forward");
  DI_REQUIRE(n_classes > 0 && max_V > 0 && max_F > 0 && H > 0 && W > 0, "render_observed: empty mesh table or image");
  DI_REQUIRE(image && depth && label, "render_observed: image, depth and label are required");
  DI_REQUIRE(class_index != nullptr && mesh_desc != nullptr, "render_observed: class_index and mesh_desc are required");
  DI_REQUIRE(normals != nullptr && light_offset != nullptr && light_intensity != nullptr && brightness_ratio != nullptr,
             "render_observed: the lit draw needs normals and the three per-sample light arrays");
  DI_REQUIRE(depth_factor > 0.f && zfar * depth_factor < 65536.f, "render_observed: zFar * depth_factor must stay below 65536");
  const MeshTable src = {(const int*)class_index, (const int*)mesh_desc, vertices, vertex_attr, normals, (const int*)faces,
                         textures, n_classes, max_V, max_F};
  const FrameOut out = {image, depth, label, nullptr, (const int*)rows, (const int*)label_value, depth_factor, N};
  const LitPerSample lit = {poses, light_offset, light_intensity, brightness_ratio};
  return frames_launch(ctx, out, src, lit, max_V, max_F, poses, K_host, B, H, W, znear, zfar);
}

// The mesh-table draw, unlit, written as decoded frames with the per-sample count of covered pixels (layout: include/deepim_hip.h).
extern "C" int deepim_render_frames_forward(deepim_ctx* ctx, uint8_t* image, uint16_t* depth, uint8_t* label, int32_t* covered,
                                            const int32_t* rows, int N, const int32_t* label_value, float depth_factor,
                                            const int32_t* class_index, const int32_t* mesh_desc, int n_classes, int max_V, int max_F,
                                            const float* vertices, const float* vertex_attr, const int32_t* faces,
                                            const float* textures, const float* poses, const float* K_host, int B, int H, int W,
                                            float znear, float zfar) {
  DI_NO_EXPORT(ctx);
  DI_DEVICE(ctx);
  DI_REQUIRE(B >= 0 && N >= B, "render_frames: the outputs need N >= B >= 0 rows");
  if (B == 0) return 0;
  DI_CAMERA(ctx, K_host, B, "deepim_render_frames_forward");
  DI_REQUIRE(n_classes > 0 && max_V > 0 && max_F > 0 && H > 0 && W > 0, "render_frames: empty mesh table or image");
  DI_REQUIRE(image && depth, "render_frames: image and depth are required");
  DI_REQUIRE(class_index != nullptr && mesh_desc != nullptr, "render_frames: class_index and mesh_desc are required");
  DI_REQUIRE(depth_factor > 0.f && zfar * depth_factor < 65536.f, "render_frames: zFar * depth_factor must stay below 65536");
  DI_REQUIRE((long)H * W <= 0x7fffffffL, "render_frames: frame too large for the int32 pixel count");
  DI_REQUIRE(B <= 65535, "render_frames: batch too large");
  const MeshTable src = {(const int*)class_index, (const int*)mesh_desc, vertices, vertex_attr, nullptr, (const int*)faces,
                         textures, n_classes, max_V, max_F};
  // the call WRITES covered: zeroed in stream order ahead of the resolve pass's adds (a memset node inside a capture)
  if (covered) DI_CHECK(hipMemsetAsync(covered, 0, (size_t)B * sizeof(int32_t), ctx->stream));
  const FrameOut out = {image, depth, label, (int*)covered, (const int*)rows, (const int*)label_value, depth_factor, N};
  return frames_launch(ctx, out, src, Unlit{}, max_V, max_F, poses, K_host, B, H, W, znear, zfar);
}

// The lit mesh-table draw of a SCENE: S slots per frame share one z-buffer plane (layout: include/deepim_hip.h).
extern "C" int deepim_render_scene_forward(deepim_ctx* ctx, uint8_t* image, uint16_t* depth, uint8_t* label, int32_t* visible,
                                           const int32_t* rows, int N, const int32_t* label_value, float depth_factor,
                                           const int32_t* class_index, const int32_t* mesh_desc, int n_classes, int max_V, int max_F,
                                           const float* vertices, const float* vertex_attr, const float* normals, const int32_t* faces,
                                           const float* textures, const float* poses, const float* K_host, const float* light_offset,
                                           const float* light_intensity, const float* brightness_ratio, int B, int S, int H, int W,
                                           float znear, float zfar) {
  DI_NO_EXPORT(ctx);
  DI_DEVICE(ctx);
  DI_REQUIRE(S >= 1 && S <= 8, "render_scene: S (slots per frame) must lie in 1..8");
  DI_REQUIRE(B >= 0 && N >= B, "render_scene: the outputs need N >= B >= 0 rows");
  DI_REQUIRE((long)B * S <= 65535, "render_scene: B * S must stay below 65536");
  DI_REQUIRE(max_F <= (1 << 24), "render_scene: a mesh of more than 2^24 triangles leaves no room for the slot in the key");
  DI_REQUIRE(depth_factor > 0.f && zfar * depth_factor < 65536.f, "render_scene: zFar * depth_factor must stay below 65536");
  if (B == 0) return 0;
  DI_REQUIRE(K_host != nullptr, "render_scene: K_host is required (the camera table is per pair, not per slot)");
  DI_REQUIRE(n_classes > 0 && max_V > 0 && max_F > 0 && H > 0 && W > 0, "render_scene: empty mesh table or image");
  DI_REQUIRE(image && depth && label, "render_scene: image, depth and label are required");
  DI_REQUIRE(class_index != nullptr && mesh_desc != nullptr && poses != nullptr, "render_scene: class_index, mesh_desc and poses are required");
  DI_REQUIRE(normals != nullptr && light_offset != nullptr && light_intensity != nullptr && brightness_ratio != nullptr,
             "render_scene: the lit draw needs normals and the three per-frame light arrays");
  DI_REQUIRE((long)H * W <= 0x7fffffffL, "render_scene: frame too large for the int32 pixel count");
  const MeshTable src = {(const int*)class_index, (const int*)mesh_desc, vertices, vertex_attr, normals, (const int*)faces,
                         textures, n_classes, max_V, max_F};
  // the call WRITES visible: zeroed in stream order ahead of the resolve pass's adds (a memset node inside a capture)
  if (visible) DI_CHECK(hipMemsetAsync(visible, 0, (size_t)B * S * sizeof(int32_t), ctx->stream));
  PV* pv;
  int rc = render_front(ctx, src, ScenePlane{S}, B, max_V, max_F, poses, K_host, B * S, H, W, znear, zfar, nullptr, &pv);
  if (rc) return rc;
  const SceneOut out = {image, depth, label, (int*)visible, (const int*)rows, (const int*)label_value, depth_factor, N, S};
  const LitPerFrame lit = {poses, light_offset, light_intensity, brightness_ratio, 0};
  const long plane = (long)H * W;
  const bool quad = plane % 4 == 0 && (((uintptr_t)image | (uintptr_t)depth | (uintptr_t)label) & 7) == 0;
  if (quad)
    hipLaunchKernelGGL(resolve_scene_kernel<4>, dim3(di_div_up(plane / 4, 256), B), dim3(256), 0, ctx->stream, out, ctx->zbuf, pv, src,
                       H, W, znear, lit);
  else
    hipLaunchKernelGGL(resolve_scene_kernel<1>, dim3(di_div_up(plane, 256), B), dim3(256), 0, ctx->stream, out, ctx->zbuf, pv, src, H,
                       W, znear, lit);
  DI_LAUNCH_CHECK();
  ctx->zbuf_dirty = 0;
  return 0;
}

// One-shot: the NEXT render entry on this context, which must draw mask_box (deepim_render_update_forward, _lit_, _classes_),
// also writes boxes (B,2,4) int32 {minx, maxx, miny, maxy}: row 0 the box of the rectangle it draws into mask_box, row 1 the box
// of its mask_rendered: what the zoom front end's bbox pass would find on the two masks. No extra launch. The request is cleared
// by that entry whether it succeeds or not; boxes == NULL withdraws it.
extern "C" int deepim_render_export_boxes(deepim_ctx* ctx, int32_t* boxes) {
  DI_REQUIRE(ctx != nullptr, "deepim_render_export_boxes: ctx is NULL");
  ctx->export_boxes = (int*)boxes;
  return 0;
}
