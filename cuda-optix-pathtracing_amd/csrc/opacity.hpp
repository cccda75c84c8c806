// opacity.hpp -- alpha cutouts (dmt_upload_opacity): the per-triangle cutout record, the A-channel lookup that
// the device and the host twin (dmt_opacity_eval) share, the brute-force pass that filters candidate hits with it and the
// leaf policy that does the same inside the BVH traversal (bvh_device.hpp: leaf_accept).
//
// Part of dmt_hip.hip's translation unit, included once after PathState and the kernel-argument accessors.  Only code
// instantiated with kFeatCutout (the *_tex_cut rows, their probes, k_aov_cut) refers to anything here, so no other kernel
// gains a register, a byte of LDS or an instruction.
//
// The rule.  A valid Moeller-Trumbore hit (t, bu, bv) on a cutout triangle counts iff alpha8 >= cutoff8, where alpha8 is the
// bilinear level-0 lookup of the opacity texture's A bytes, as floats in [0, 255], at the hit's UV.  The decision is a pure
// function of (triangle, bu, bv): brute force and the BVH produce those bit for bit, so they cut the same hits.
#pragma once

// One record per triangle, 32 B = two 16-byte loads (BVH leaf, per lane) or one s_load_dwordx8 (brute force, wave-uniform
// triangle).  wh == 0 marks a triangle of an opaque material: the second half alone decides that, so a candidate hit on a
// solid triangle costs ONE 16-byte load in a leaf and one prefetched dword in the brute-force loop.  A cutout triangle has
// everything the lookup needs right here -- no walk triangle -> material -> texture -> descriptor -- and then reads its four
// texels.
struct OpacityRec {
  float u0, v0, u1, v1;
  float u2, v2;
  uint32_t first;  // first texel of the opacity texture in the RGBA8 store
  uint32_t wh;     // width | height << 16 (both <= 65535, checked at upload); 0 = opaque
};
static_assert(sizeof(OpacityRec) == 32, "cutout record size");

// alpha8 of the texture (first, w, h) in `rgba` at UV (s, t): tex_bilinear's level-0 arithmetic (mirror wrap, x = s*w - 0.5,
// floorf, the same lerp order) on the raw A bytes as floats, fp32, nothing contracted.  x and y are clamped to +-2^30 before
// the conversion to int, so every input -- NaN and infinities included -- reads inside the texture; UVs that
// dmt_upload_opacity admits (|uv| <= 2^20, textures up to 1024 texels wide) never reach the clamp.
template <class Texels>
DMT_HD float opacity_alpha8(Texels rgba, uint32_t first, int w, int h, float s, float t) {
#pragma clang fp contract(off)
  auto mirror = [](int c, int size) {
    int const p = size * 2;
    c %= p;
    if (c < 0) c += p;
    return c < size ? c : (p - c - 1);
  };
  float const lim = 1073741824.f;
  float const x = __builtin_fminf(__builtin_fmaxf(s * float(w) - 0.5f, -lim), lim);
  float const y = __builtin_fminf(__builtin_fmaxf(t * float(h) - 0.5f, -lim), lim);
  float const fx = __builtin_floorf(x), fy = __builtin_floorf(y);
  int const x0 = int(fx), y0 = int(fy);
  float const tx = x - fx, ty = y - fy;
  int const xa = mirror(x0, w), xb = mirror(x0 + 1, w), ya = mirror(y0, h), yb = mirror(y0 + 1, h);
  size_t const ra = size_t(first) + size_t(ya) * size_t(w), rb = size_t(first) + size_t(yb) * size_t(w);
  float const a00 = float(rgba[ra + size_t(xa)] >> 24), a10 = float(rgba[ra + size_t(xb)] >> 24);
  float const a01 = float(rgba[rb + size_t(xa)] >> 24), a11 = float(rgba[rb + size_t(xb)] >> 24);
  float const ax0 = a00 * (1.f - tx) + a10 * tx, ax1 = a01 * (1.f - tx) + a11 * tx;
  return ax0 * (1.f - ty) + ax1 * ty;
}
// the hit's UV in ONE fixed order: w0 = (1 - bu) - bv, s = (w0*u0 + bu*u1) + bv*u2 (t alike), every operation rounded
DMT_HD void opacity_uv(float u0, float v0, float u1, float v1, float u2, float v2, float bu, float bv, float& s, float& t) {
#pragma clang fp contract(off)
  float const w0 = (1.f - bu) - bv;
  s = (w0 * u0 + bu * u1) + bv * u2;
  t = (w0 * v0 + bu * v1) + bv * v2;
}
// alpha8 of a cutout record's triangle at (bu, bv)
template <class Texels>
DMT_HD float opacity_alpha8_at(Texels rgba, OpacityRec const& R, float bu, float bv) {
  float s, t;
  opacity_uv(R.u0, R.v0, R.u1, R.v1, R.u2, R.v2, bu, bv, s, t);
  return opacity_alpha8(rgba, R.first, int(R.wh & 0xFFFFu), int(R.wh >> 16), s, t);
}

// what a cutout launch reads beside the scene (RenderParams::opacity / texRgba / opacityCutoff8), fetched where it is needed
struct CutoutView {
  OpacityRec const* recs;
  uint32_t const* rgba;
  float cutoff8;
};
DMT_DEV CutoutView load_cutout(KArgs k) {
  k = kargs(k);
  return CutoutView{k->opacity, k->texRgba, k->opacityCutoff8};
}

// ---- BVH: the cutout leaf policy.  The pair test is the static one; each half that would be accepted is filtered first.
// Per lane: the second half of the triangle's record (one 16-byte load) says opaque or not; a cutout triangle loads the
// first half and its four texels.
struct LeafCutout {
  CutoutView cv;
};
DMT_DEV PairHit pair_test_at(BvhView const& bv, uint32_t idx, f3 o, f3 d, LeafCutout const&) { return pair_test(bv.pairs + idx, o, d); }
DMT_DEV bool leaf_accept(LeafCutout const& m, uint32_t orig, float bu, float bv) {
  float4 const* const q = reinterpret_cast<float4 const*>(m.cv.recs + orig);
  float4 const hi = q[1];  // u2 v2 first wh
  uint32_t const wh = __float_as_uint(hi.w);
  if (wh == 0u) return true;
  float4 const lo = q[0];
  OpacityRec R;
  R.u0 = lo.x, R.v0 = lo.y, R.u1 = lo.z, R.v1 = lo.w, R.u2 = hi.x, R.v2 = hi.y, R.first = __float_as_uint(hi.z), R.wh = wh;
  return opacity_alpha8_at(m.cv.rgba, R, bu, bv) >= m.cv.cutoff8;
}

// ---- brute force: trace_pair_brute<false> with the cutout rule.  The plain loop over every triangle (the culled clusters
// stay with the solid rows).  The triangle is wave-uniform: its cutout word arrives with the scalar prefetch of the triangle
// record (one more SGPR per ping-pong set) and the branch on it is wave-uniform, so a solid triangle runs the solid test.
// For a cutout triangle the record comes by one scalar load and only the lanes whose candidate already passed
// valid && t < best (closest) or valid && t < smax (shadow) look the texture up, the two rays of the lane one after the
// other through one copy of the lookup.
DMT_DEV void cutout_pass_pair(CutoutView const& cv, OpacityRec const DMT_CONST_AS* rec, v2f uu, v2f vv, bool& c1, bool& c2) {
  OpacityRec R;
  R.u0 = rec->u0, R.v0 = rec->v0, R.u1 = rec->u1, R.v1 = rec->v1, R.u2 = rec->u2, R.v2 = rec->v2, R.first = rec->first, R.wh = rec->wh;
#pragma nounroll
  for (int r = 0; r < 2; ++r) {
    bool const want = r ? c2 : c1;
    if (want) {
      bool const pass = opacity_alpha8_at(cv.rgba, R, r ? uu.y : uu.x, r ? vv.y : vv.x) >= cv.cutoff8;
      if (r) c2 = pass;
      else c1 = pass;
    }
  }
}
#define DMT_TRI_TEST_CUT(P, cw, idx)                                                                            \
  do {                                                                                                         \
    MTPair m;                                                                                                  \
    mt_core9<v2f>(P##0, P##1, P##2, P##3, P##4, P##5, P##6, P##7, P##8, st.rp.ox, st.rp.oy, st.rp.oz, st.rp.dx, \
                  st.rp.dy, st.rp.dz, m.det, m.t, m.u, m.v);                                                   \
    bool c1 = doC && mt_valid(m.det.x, m.t.x, m.u.x, m.v.x) && m.t.x < bestT; /* strict <: lowest index wins */ \
    bool c2 = doS && mt_valid(m.det.y, m.t.y, m.u.y, m.v.y) && m.t.y < st.smax;                                \
    if (cw != 0u) {                                                                                            \
      if (__any(c1 || c2)) cutout_pass_pair(cv, recs + (idx), m.u, m.v, c1, c2);                               \
    }                                                                                                          \
    if (c1) {                                                                                                  \
      bestT = m.t.x;                                                                                           \
      bestTri = int(idx);                                                                                      \
      bu = m.u.x;                                                                                              \
      bv = m.v.x;                                                                                              \
    }                                                                                                          \
    if (c2) occluded = true;                                                                                   \
  } while (0)
// bt (optional): the t of the winning hit
DMT_DEV void trace_pair_brute_cut(KArgs k, PathState const& st, bool doC, bool doS, int& bestTri, float& bu, float& bv, bool& occluded,
                                  float* bt = nullptr) {
  k = kargs(k);
  auto const* tris = to_const_as(k->scene.tris);
  auto const* recs = to_const_as(k->opacity);
  CutoutView const cv = load_cutout(k);
  uint32_t const n = k->scene.triCount;
  uint32_t const last = n ? n - 1 : 0;
  float bestT = kInf;
  bestTri = -1, bu = 0.f, bv = 0.f, occluded = false;
  DMT_TRI_DECL(a);
  DMT_TRI_DECL(b);
  uint32_t ca, cb;
  DMT_TRI_LOAD(a, 0);  // both arrays always hold >= 1 record (DevBuf::assign)
  ca = recs[0].wh;
  for (uint32_t i = 0; i < n;) {
    uint32_t const ib = i + 1 < last ? i + 1 : last;
    DMT_TRI_LOAD(b, ib);
    cb = recs[ib].wh;
    __builtin_amdgcn_sched_barrier(0);  // keep the prefetch s_loads above the arithmetic
    DMT_TRI_TEST_CUT(a, ca, i);
    if (++i >= n) break;
    uint32_t const ia = i + 1 < last ? i + 1 : last;
    DMT_TRI_LOAD(a, ia);
    ca = recs[ia].wh;
    __builtin_amdgcn_sched_barrier(0);
    DMT_TRI_TEST_CUT(b, cb, i);
    ++i;
  }
  if (bt) *bt = bestT;
}

// the two traversals of trace_pair_bvh with the cutout leaf policy.  bt (optional): the closest hit's t
DMT_DEV void trace_pair_bvh_cut(KArgs k, PathState const& st, bool doC, bool doS, uint32_t gtid, int& bestTri, float& bu, float& bv,
                                bool& occluded, float* btOut = nullptr) {
  BvhView const bvh = load_bvh(k);
  LeafCutout const lc{load_cutout(k)};
  float bt;
  bvh_closest<false>(bvh, doC, mk3(st.rp.ox.x, st.rp.oy.x, st.rp.oz.x), mk3(st.rp.dx.x, st.rp.dy.x, st.rp.dz.x), gtid, bestTri, bt, bu, bv,
                     nullptr, lc);
  occluded = bvh_any<false>(bvh, doS, mk3(st.rp.ox.y, st.rp.oy.y, st.rp.oz.y), mk3(st.rp.dx.y, st.rp.dy.y, st.rp.dz.y), st.smax, gtid,
                            nullptr, lc);
  if (btOut) *btOut = bt;
}
