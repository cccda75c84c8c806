// motion.hpp -- motion blur on the device (dmt_set_motion): the sample times of a lane, the brute-force pass
// over triangles rebuilt at those times, and the post-hit record of a moving triangle.  The leaf step of the motion tree is
// bvh_device.hpp's (pair_test_motion); what the host and the device share (shutter_time, motion_lerp) is pt_device.hpp's.
//
// Part of dmt_hip.hip's translation unit, included once after PathState and the kernel-argument accessors.  Only code
// instantiated with kFeatMotion (the *_motion rows, their probes, k_aov_motion) refers to anything here, so no other
// kernel gains a register, a byte of LDS or an instruction.
//
// The triangle at time t, once for every path: A = the key-0 TriIsect, D = B - A made on the host (B = packTriangle of
// key 1), the tested triangle = fmaf(t, D, A) field by field.  Brute force reads A and D of the wave-uniform triangle
// through scalar loads; a leaf of the motion tree reads the same numbers from the interleaved pair records.  Same inputs,
// same single fmaf, same Moeller-Trumbore core: bit-identical (t, u, v), as for static triangles.
#pragma once

// Times of a lane's samples, [slot][thread], in LDS like the other cold per-lane values: 0 = the sample whose path the lane
// extends, 1 = the sample its pending shadow ray belongs to, 2 = the prepared (next) sample.  Slots 0 and 1 differ exactly
// when a path ended with its last shadow ray untraced and the lane started the next sample beside it (PathState, finPending);
// that is why the brute-force pass builds a triangle per ray (packed: one v_pk_fma_f32 per field for both) and not per lane.
__shared__ float s_motionT[3 * kLdsThreads];
DMT_DEV float motion_time() { return s_motionT[threadIdx.x]; }
DMT_DEV float motion_time_shadow() { return s_motionT[kLdsThreads + threadIdx.x]; }
DMT_DEV void motion_set_time(float t) { s_motionT[threadIdx.x] = t; }
DMT_DEV void motion_park_shadow() { s_motionT[kLdsThreads + threadIdx.x] = s_motionT[threadIdx.x]; }
DMT_DEV void motion_set_prepared(float t) { s_motionT[2 * kLdsThreads + threadIdx.x] = t; }
DMT_DEV void motion_begin_prepared() { s_motionT[threadIdx.x] = s_motionT[2 * kLdsThreads + threadIdx.x]; }

// the time of sample s of the pixel whose sample 0 has Halton index pixBase, under the launch's shutter
DMT_DEV float motion_sample_time(KArgs k, int32_t pixBase, uint32_t s) {
  k = kargs(k);
  int32_t const hidx = pixBase + int32_t(s) * (k->sp.scale0 * k->sp.scale1);
  return shutter_time(uint32_t(hidx), k->motion.open, k->motion.close);
}

// trace_pair_brute<false> over triangles at the rays' times: time.x for the closest-hit ray, time.y for the shadow ray.
// The plain loop over every triangle: the culled clusters' bounds are of key 0.  A and D arrive by s_load, prefetched one
// triangle ahead as in the static loop (36 SGPRs for the two ping-pong sets); nine v_pk_fma_f32 make the two rays' triangles.
// bt (optional): the t of the winning hit.
#define DMT_TRI_TEST_MOTION(P, Q, idx)                                                                             \
  do {                                                                                                             \
    v2f det, tt, uu, vv;                                                                                           \
    mt_core9_vv(fma_(time, Q##0, v2f{P##0, P##0}), fma_(time, Q##1, v2f{P##1, P##1}), fma_(time, Q##2, v2f{P##2, P##2}), \
                fma_(time, Q##3, v2f{P##3, P##3}), fma_(time, Q##4, v2f{P##4, P##4}), fma_(time, Q##5, v2f{P##5, P##5}), \
                fma_(time, Q##6, v2f{P##6, P##6}), fma_(time, Q##7, v2f{P##7, P##7}), fma_(time, Q##8, v2f{P##8, P##8}), \
                st.rp.ox, st.rp.oy, st.rp.oz, st.rp.dx, st.rp.dy, st.rp.dz, det, tt, uu, vv);                      \
    bool const v1 = mt_valid(det.x, tt.x, uu.x, vv.x);                                                             \
    bool const v2 = mt_valid(det.y, tt.y, uu.y, vv.y);                                                             \
    if (doC && v1 && tt.x < bestT) { /* strict <: lowest index wins ties, as the static loop */                     \
      bestT = tt.x;                                                                                                \
      bestTri = int(idx);                                                                                          \
      bu = uu.x;                                                                                                   \
      bv = vv.x;                                                                                                   \
    }                                                                                                              \
    if (doS && v2 && tt.y < st.smax) occluded = true;                                                              \
  } while (0)
#define DMT_TRI_DECL_M(P) float P##0, P##1, P##2, P##3, P##4, P##5, P##6, P##7, P##8
#define DMT_TRI_LOAD_M(P, arr, idx)                                                                          \
  P##0 = arr[idx].p0x, P##1 = arr[idx].p0y, P##2 = arr[idx].p0z, P##3 = arr[idx].e0x, P##4 = arr[idx].e0y, \
  P##5 = arr[idx].e0z, P##6 = arr[idx].e1x, P##7 = arr[idx].e1y, P##8 = arr[idx].e1z
DMT_DEV void trace_pair_brute_motion(KArgs k, PathState const& st, bool doC, bool doS, v2f time, int& bestTri, float& bu, float& bv,
                                     bool& occluded, float* bt = nullptr) {
  k = kargs(k);
  auto const* tris = to_const_as(k->scene.tris);
  auto const* dts = to_const_as(k->motion.dtris);
  uint32_t const n = k->scene.triCount;
  uint32_t const last = n ? n - 1 : 0;
  float bestT = kInf;
  bestTri = -1, bu = 0.f, bv = 0.f, occluded = false;
  DMT_TRI_DECL_M(a);
  DMT_TRI_DECL_M(da);
  DMT_TRI_DECL_M(b);
  DMT_TRI_DECL_M(db);
  DMT_TRI_LOAD_M(a, tris, 0);  // both arrays always hold >= 1 record (DevBuf::assign)
  DMT_TRI_LOAD_M(da, dts, 0);
  for (uint32_t i = 0; i < n;) {
    uint32_t const ib = i + 1 < last ? i + 1 : last;
    DMT_TRI_LOAD_M(b, tris, ib);
    DMT_TRI_LOAD_M(db, dts, ib);
    __builtin_amdgcn_sched_barrier(0);  // keep the prefetch s_loads above the arithmetic
    DMT_TRI_TEST_MOTION(a, da, i);
    if (++i >= n) break;
    uint32_t const ia = i + 1 < last ? i + 1 : last;
    DMT_TRI_LOAD_M(a, tris, ia);
    DMT_TRI_LOAD_M(da, dts, ia);
    __builtin_amdgcn_sched_barrier(0);
    DMT_TRI_TEST_MOTION(b, db, i);
    ++i;
  }
  if (bt) *bt = bestT;
}

// The post-hit record of triangle `tri` at time t: p_i(t) = fmaf(t, P1_i - P0_i, P0_i) (motion_lerp; dmt_motion_positions is
// its host twin, bit for bit) and the geometric normal normalize(cross(e1, e0)) of those vertices in packTriangle's order
// of operations, without contraction, the inverse length by v_rsq_f32.  Material id and the rest are key 0's.
DMT_DEV TriPost motion_post(KArgs k, TriPost P, int tri, float t) {
#pragma clang fp contract(off)
  TriKey1 const Q = kargs(k)->motion.post1[tri];
  P.p0x = motion_lerp(t, P.p0x, Q.p0x), P.p0y = motion_lerp(t, P.p0y, Q.p0y), P.p0z = motion_lerp(t, P.p0z, Q.p0z);
  P.p1x = motion_lerp(t, P.p1x, Q.p1x), P.p1y = motion_lerp(t, P.p1y, Q.p1y), P.p1z = motion_lerp(t, P.p1z, Q.p1z);
  P.p2x = motion_lerp(t, P.p2x, Q.p2x), P.p2y = motion_lerp(t, P.p2y, Q.p2y), P.p2z = motion_lerp(t, P.p2z, Q.p2z);
  float const e0x = P.p1x - P.p0x, e0y = P.p1y - P.p0y, e0z = P.p1z - P.p0z;
  float const e1x = P.p2x - P.p0x, e1y = P.p2y - P.p0y, e1z = P.p2z - P.p0z;
  float const cx = e1y * e0z - e1z * e0y, cy = e1z * e0x - e1x * e0z, cz = e1x * e0y - e1y * e0x;  // cross(e1, e0)
  float const inv = rsqrt_ieee((cx * cx + cy * cy) + cz * cz);
  P.nx = cx * inv, P.ny = cy * inv, P.nz = cz * inv;
  return P;
}

