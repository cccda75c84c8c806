// tri_records.hpp -- the two per-triangle records of the render kernels and the one function that makes them.
//
// packTriangle is __host__ __device__: dmt_upload_triangles and dmt_update_vertices run it on the host, the record kernel
// of dmt_update_vertices_device (bvh_gpu_build.hip, compiled without contraction, with IEEE division and square root) runs it
// on the device, and the records agree byte for byte for every triangle of non-zero area (a zero-area triangle's NaN normal
// may differ in payload).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DMT_HD __host__ __device__
#else
#define DMT_HD
#endif

namespace dmt {

// hot-loop triangle record, built at upload: p0, e0 = p1-p0, e1 = p2-p0 (same float
// subtractions the reference does per test, CC/private/shapes.cu:10-11)
struct TriIsect {  // 48 B, three 16-byte loads
  float p0x, p0y, p0z, e0x;
  float e0y, e0z, e1x, e1y;
  float e1z;
  uint32_t matId;
  uint32_t pad0, pad1;
};
// post-hit record: original vertices (error bound needs them) + unit geometric normal
// normalize(cross(e1,e0)) precomputed with the same IEEE expression (shapes.cu:48)
struct TriPost {  // 64 B
  float p0x, p0y, p0z, p1x;
  float p1y, p1z, p2x, p2y;
  float p2z, nx, ny, nz;
  uint32_t matId, pad0, pad1, pad2;
};

// motion blur (dmt_set_motion): the key-1 vertices of a triangle, what the post-hit record of a moving
// triangle is rebuilt from.  (The intersection side keeps a second TriIsect array: D = B - A, field by field.)
struct TriKey1 {  // 48 B
  float p0x, p0y, p0z, p1x;
  float p1y, p1z, p2x, p2y;
  float p2z, pad0, pad1, pad2;
};

// both records of the triangle with vertices v[0..2], v[3..5], v[6..8]
DMT_HD inline void packTriangle(float const v[9], uint32_t matId, TriIsect& t, TriPost& q) {
  float const e0x = v[3] - v[0], e0y = v[4] - v[1], e0z = v[5] - v[2];
  float const e1x = v[6] - v[0], e1y = v[7] - v[1], e1z = v[8] - v[2];
  float const cx = e1y * e0z - e1z * e0y, cy = e1z * e0x - e1x * e0z, cz = e1x * e0y - e1y * e0x;  // cross(e1, e0)
  float const inv = 1.0f / ::sqrtf(cx * cx + cy * cy + cz * cz);
  t.p0x = v[0], t.p0y = v[1], t.p0z = v[2];
  t.e0x = e0x, t.e0y = e0y, t.e0z = e0z;
  t.e1x = e1x, t.e1y = e1y, t.e1z = e1z;
  t.matId = matId, t.pad0 = 0, t.pad1 = 0;
  q.p0x = v[0], q.p0y = v[1], q.p0z = v[2];
  q.p1x = v[3], q.p1y = v[4], q.p1z = v[5];
  q.p2x = v[6], q.p2y = v[7], q.p2z = v[8];
  q.nx = cx * inv, q.ny = cy * inv, q.nz = cz * inv;
  q.matId = matId, q.pad0 = q.pad1 = q.pad2 = 0;
}

}  // namespace dmt
