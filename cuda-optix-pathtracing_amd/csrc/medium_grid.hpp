// medium_grid.hpp -- the heterogeneous medium (dmt_set_medium_grid): a regular grid of densities that fills
// the medium's box, piecewise constant, marched exactly by a 3-D DDA.  include/dmt_hip.h states the definition for callers.
//
// Part of dmt_hip.hip's translation unit, included once after medium.hpp.  This file is what the device (the *_medium_grid
// rows, the probe dmt_test_medium_grid) and the host twin (dmt_medium_grid_march) share, one body, the way medium_segment is
// shared; medium_device.hpp holds the callers inside path_shade.
#pragma once

namespace dmt {

constexpr int kMediumGridMaxAxis = 512;                   // voxels per axis
constexpr uint64_t kMediumGridMaxVoxels = uint64_t(1) << 26;

struct MediumGridParams {  // the tail of RenderParams after MediumParams; density == nullptr in every launch without a grid
  float const* density;    // n[0] * n[1] * n[2] values, x fastest
  int32_t n[3];
  float cell[3], invCell[3];
  int32_t imin[3], imax[3];  // the support: the inclusive index range of voxels with density > 0, per axis
  float slo[3], shi[3];      // its planes plane(a, imin[a]), plane(a, imax[a] + 1)
};

// the position of plane i (0 .. n) of an axis: multiply, then add; the last plane is the box's own
__host__ __device__ inline float medium_grid_plane(float lo, float hi, float cell, int n, int i) {
#pragma clang fp contract(off)
  float const p = float(i) * cell;
  return i == n ? hi : lo + p;
}

// cell, invCell and the support planes of a grid of g.n voxels with support [g.imin, g.imax] in the box [lo, hi] (host, on
// upload and whenever dmt_set_medium changes the box)
inline void medium_grid_derive(MediumGridParams& g, float const* lo, float const* hi) {
#pragma clang fp contract(off)
  for (int a = 0; a < 3; ++a) {
    g.cell[a] = (hi[a] - lo[a]) / float(g.n[a]);
    g.invCell[a] = medium_rcp(g.cell[a]);
    g.slo[a] = medium_grid_plane(lo[a], hi[a], g.cell[a], g.n[a], g.imin[a]);
    g.shi[a] = medium_grid_plane(lo[a], hi[a], g.cell[a], g.n[a], g.imax[a] + 1);
  }
}

struct MediumGridMarch {
  float tau;      // the optical depth of the segment (no collision), or what was gathered before the colliding voxel
  float ts;       // the collision parameter, when one happened
  int collided, steps;
};

// the entry index of one axis: clamp(floorf((p - lo) * invCell), imin, imax); a NaN lands on imin
__host__ __device__ inline int medium_grid_entry(float p, float lo, float invCell, int imin, int imax) {
#pragma clang fp contract(off)
  float const f = __builtin_floorf((p - lo) * invCell);
  float const c = !(f >= float(imin)) ? float(imin) : (f > float(imax) ? float(imax) : f);
  return int(c);
}

// The optical depth of the ray o + t d over 0 <= t <= tEnd through the grid, up to the point where it reaches tauTarget
// (+inf: never).  fp32, no contraction, one order of operations; the three axes are written out, so that nothing is an
// indexed private array.  lo, hi: the medium's box.  At most n[0] + n[1] + n[2] iterations: every iteration but the last
// moves one index one voxel on inside the support range, and never back.
__host__ __device__ inline MediumGridMarch medium_grid_march(float const* o, float const* d, float tEnd, float tauTarget, float sigmaT,
                                                             float const* lo, float const* hi, MediumGridParams const& g) {
#pragma clang fp contract(off)
  MediumGridMarch r;
  r.tau = 0.0f, r.ts = 0.0f, r.collided = 0, r.steps = 0;
  float t0, t1;
  if (!medium_segment(o, d, tEnd, g.slo, g.shi, &t0, &t1)) return r;
  float const inf = __builtin_huge_valf();
  bool const px = __builtin_fabsf(d[0]) < kMediumParallel, py = __builtin_fabsf(d[1]) < kMediumParallel, pz = __builtin_fabsf(d[2]) < kMediumParallel;
  float const invx = px ? 0.0f : medium_rcp(d[0]), invy = py ? 0.0f : medium_rcp(d[1]), invz = pz ? 0.0f : medium_rcp(d[2]);
  int const sx = d[0] > 0.0f ? 1 : -1, sy = d[1] > 0.0f ? 1 : -1, sz = d[2] > 0.0f ? 1 : -1;
  int ix = medium_grid_entry(o[0] + t0 * d[0], lo[0], g.invCell[0], g.imin[0], g.imax[0]);
  int iy = medium_grid_entry(o[1] + t0 * d[1], lo[1], g.invCell[1], g.imin[1], g.imax[1]);
  int iz = medium_grid_entry(o[2] + t0 * d[2], lo[2], g.invCell[2], g.imin[2], g.imax[2]);
  // The exit parameter of the current voxel per axis, from the plane index every time and never accumulated; only the axis
  // that stepped has a new one.  The density of the voxel stepped into is loaded before the current one is used, so that
  // the gather of one iteration is in flight during the arithmetic of the next (at most 2^26 voxels: 32-bit indices).
  float tnx = px ? inf : (medium_grid_plane(lo[0], hi[0], g.cell[0], g.n[0], ix + (sx > 0 ? 1 : 0)) - o[0]) * invx;
  float tny = py ? inf : (medium_grid_plane(lo[1], hi[1], g.cell[1], g.n[1], iy + (sy > 0 ? 1 : 0)) - o[1]) * invy;
  float tnz = pz ? inf : (medium_grid_plane(lo[2], hi[2], g.cell[2], g.n[2], iz + (sz > 0 ? 1 : 0)) - o[2]) * invz;
  int32_t const strideY = sy * g.n[0], strideZ = sz * g.n[0] * g.n[1];
  int32_t voxel = (iz * g.n[1] + iy) * g.n[0] + ix;
  float density = g.density[voxel];
  float tc = t0, tau = 0.0f;
  int steps = 0;
  for (;;) {
    ++steps;
    int ax = 0;
    float tn = tnx;
    if (tny < tn) ax = 1, tn = tny;
    if (tnz < tn) ax = 2, tn = tnz;
    float const te = tn < t1 ? tn : t1;
    float seg = te - tc;
    if (!(seg > 0.0f)) seg = 0.0f;
    // the voxel after this one: there is one while tn < t1 and the step stays inside the support
    bool more = tn < t1;
    if (ax == 0) {
      ix += sx, voxel += sx;
      more = more && ix >= g.imin[0] && ix <= g.imax[0];
      tnx = (medium_grid_plane(lo[0], hi[0], g.cell[0], g.n[0], ix + (sx > 0 ? 1 : 0)) - o[0]) * invx;
    } else if (ax == 1) {
      iy += sy, voxel += strideY;
      more = more && iy >= g.imin[1] && iy <= g.imax[1];
      tny = (medium_grid_plane(lo[1], hi[1], g.cell[1], g.n[1], iy + (sy > 0 ? 1 : 0)) - o[1]) * invy;
    } else {
      iz += sz, voxel += strideZ;
      more = more && iz >= g.imin[2] && iz <= g.imax[2];
      tnz = (medium_grid_plane(lo[2], hi[2], g.cell[2], g.n[2], iz + (sz > 0 ? 1 : 0)) - o[2]) * invz;
    }
    float densityNext = 0.0f;
    if (more) densityNext = g.density[voxel];
    float const s = sigmaT * density;
    float const dtau = s * seg;
    if (s > 0.0f && tau + dtau >= tauTarget) {
      double q = double(tauTarget - tau) / double(s);
#if defined(__HIP_DEVICE_COMPILE__)
      asm("" : "+v"(q));  // (as in medium_rcp: keeps the quotient in double)
#endif
      float const ts = tc + float(q);
      r.ts = ts < te ? ts : te;
      r.collided = 1;
      break;
    }
    tau += dtau;
    tc = tc > te ? tc : te;
    if (!more) break;
    density = densityNext;
  }
  r.tau = tau, r.steps = steps;
  return r;
}

// dmt_set_medium_grid_device: the support index ranges, the number of voxels > 0, the largest density and the first voxel
// that is negative or not finite, reduced over a grid in device memory.  words: {min x, min y, min z, max x, max y, max z,
// count, bits of the largest density, first invalid voxel}, initialised to {~0 x 3, 0 x 3, 0, 0, ~0}.
#if defined(__HIPCC__)
__global__ void k_medium_grid_scan(float const* density, int nx, int ny, uint32_t total, uint32_t* words) {
  uint32_t const stride = gridDim.x * blockDim.x;
  uint32_t lo0 = ~0u, lo1 = ~0u, lo2 = ~0u, hi0 = 0u, hi1 = 0u, hi2 = 0u, count = 0u, top = 0u, bad = ~0u;  // the thread's own share
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < total; v += stride) {
    float const x = density[v];
    if (!(x >= 0.0f) || !(x < __builtin_huge_valf())) {
      bad = min(bad, v);
    } else if (x > 0.0f) {
      uint32_t const ix = v % uint32_t(nx), iy = (v / uint32_t(nx)) % uint32_t(ny), iz = v / (uint32_t(nx) * uint32_t(ny));
      lo0 = min(lo0, ix), lo1 = min(lo1, iy), lo2 = min(lo2, iz);
      hi0 = max(hi0, ix), hi1 = max(hi1, iy), hi2 = max(hi2, iz);
      ++count;
      top = max(top, __float_as_uint(x));  // (ordered as the floats are: x > 0)
    }
  }
  if (bad != ~0u) atomicMin(&words[8], bad);
  if (count) {
    atomicMin(&words[0], lo0), atomicMin(&words[1], lo1), atomicMin(&words[2], lo2);
    atomicMax(&words[3], hi0), atomicMax(&words[4], hi1), atomicMax(&words[5], hi2);
    atomicAdd(&words[6], count);
    atomicMax(&words[7], top);
  }
}
#endif

}  // namespace dmt
