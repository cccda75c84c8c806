// dmt_fbx.cpp -- binary FBX mesh reader, replacing the FBX SDK call of the reference's
// MeshFbxParser::ImportFBX (src/core/private/core-mesh-parser.cpp:617-687; declared
// src/core/public/core-mesh-parser.h:15-24), which this image does not have.
//
// Reads what that function uses: the FIRST mesh geometry of the file (Objects/Geometry "Mesh": Vertices,
// PolygonVertexIndex), triangulated as fans, with the local transform of the Model it is connected to
// (Properties70: Lcl Translation / Lcl Rotation (Euler XYZ, degrees) / Lcl Scaling) and the file's unit scale
// brought to centimetres (GlobalSettings/UnitScaleFactor), as ImportFBX does with FbxSystemUnit::cm.ConvertScene.
// File format (Kaydara binary, versions 7100-7400: 32-bit record offsets; 7500+: 64-bit): 27-byte header, then
// nested node records {end offset, property count, property bytes, name, properties, children, 13/25-byte null
// record}; array properties (f d l i b) may be zlib-deflated.
//
// Axis system (core-mesh-parser.cpp:630-655).  ImportFBX converts the scene to FbxAxisSystem(eZAxis, eParityOdd,
// eLeftHanded) before it bakes the node's global transform into the vertices.  In that system the UP vector is +Z, the
// FRONT vector (FBX: the axis that points towards the viewer) is the second of the two remaining axes, +Y, and the third
// ("coord") axis is X; a right-handed system has coord = up x front (Maya: Y x Z = +X; 3ds Max: Z x -Y = +X), so the
// left-handed target has coord = -(Z x Y) = +X.  A file states its own system in GlobalSettings: UpAxis / UpAxisSign,
// FrontAxis / FrontAxisSign, CoordAxis / CoordAxisSign (axis indices 0..2 and signs), i.e. three signed unit vectors
// r (coord), u (up), f (front) in file coordinates.  The change of basis that carries each of them onto the target's
// is  p' = ((p . r), (p . f), (p . u)):  a point keeps its "right / up / front" amounts.  When the file is right-handed
// (det[r u f] = +1) that map is a reflection, so the triangles' winding is reversed with it (v1 <-> v2, UVs alike) to
// keep outward faces outward; Blender's exports (Z up, -Y front, X coord: scenes/sphere.fbx, scenes/teapot.fbx) become
// (x, -y, z).  DECISION, unpinned: whether the SDK's ConvertScene really mirrors geometry on a handedness change (it is
// documented to edit node transforms only) cannot be checked without the SDK; this reader does what the requested target
// system MEANS.  A file without these properties is taken as already in the target system (this repo's older fixtures).
// One observation that speaks against it and is recorded rather than acted on: scenes/scene_test.json turns teapot.fbx
// (Y up, +Z front, right-handed) by 180 degrees about x and puts it at z = -1.32 under a camera that looks slightly down;
// with this reading the teapot stands along +z after the import, so the scene shows it upside down in the lower half of
// the frame (profiles/r03/teapot_scene_test_*.png), whereas an import that left its height along -z would frame it upright
// and centred.  No definition of the requested axis system yields that map, so it is not guessed at.
// NOT reproduced: pre/post rotations, pivots, geometric transforms, parent chains, instancing, animation.  Parity
// unpinned: no FBX SDK, no reference-side vectors; tested against files written by this repo's own writer
// (tools/make_fbx_fixture.py, three axis systems) and against the structure of the reference's scenes/sphere.fbx.
#include <zlib.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "dmt_scene.hpp"

namespace dmt_host {
namespace {

struct Prop {
  char type = 0;
  double num = 0;             // scalar types
  std::string str;            // S / R
  std::vector<double> arr;    // array types, widened
};
struct Node {
  std::string name;
  std::vector<Prop> props;
  std::vector<Node> children;
  Node const* child(char const* n) const {
    for (auto const& c : children)
      if (c.name == n) return &c;
    return nullptr;
  }
};

struct Reader {
  std::vector<unsigned char> d;
  bool wide = false;  // 64-bit offsets (version >= 7500)
  std::string err;

  template <class T>
  bool get(size_t o, T& v) {
    if (o + sizeof(T) > d.size()) return err = "truncated file", false;
    memcpy(&v, &d[o], sizeof(T));
    return true;
  }
  bool readProps(size_t& o, uint64_t count, std::vector<Prop>& out) {
    for (uint64_t i = 0; i < count; ++i) {
      if (o >= d.size()) return err = "truncated properties", false;
      Prop p;
      p.type = char(d[o++]);
      switch (p.type) {
        case 'Y': { int16_t v; if (!get(o, v)) return false; p.num = v, o += 2; break; }
        case 'C': { if (o >= d.size()) return err = "truncated", false; p.num = d[o], o += 1; break; }
        case 'I': { int32_t v; if (!get(o, v)) return false; p.num = v, o += 4; break; }
        case 'F': { float v; if (!get(o, v)) return false; p.num = v, o += 4; break; }
        case 'D': { double v; if (!get(o, v)) return false; p.num = v, o += 8; break; }
        case 'L': { int64_t v; if (!get(o, v)) return false; p.num = double(v), o += 8; break; }
        case 'S': case 'R': {
          uint32_t len;
          if (!get(o, len)) return false;
          o += 4;
          if (o + len > d.size()) return err = "truncated string", false;
          p.str.assign(reinterpret_cast<char const*>(&d[o]), len);
          o += len;
          break;
        }
        case 'f': case 'd': case 'l': case 'i': case 'b': {
          uint32_t n, enc, clen;
          if (!get(o, n) || !get(o + 4, enc) || !get(o + 8, clen)) return false;
          o += 12;
          if (o + clen > d.size()) return err = "truncated array", false;
          size_t const esz = p.type == 'f' || p.type == 'i' ? 4 : (p.type == 'b' ? 1 : 8);
          // the element count comes from the file: bound it by what the stored bytes can possibly hold BEFORE allocating
          // (raw: exactly clen bytes; deflate expands at most ~1032:1) and by an absolute limit of 2^28 elements
          uint64_t const need = uint64_t(n) * esz;
          if (n > (1u << 28) || (enc == 0 && need != clen) || (enc == 1 && need > uint64_t(clen) * 1032u + 64u) || enc > 1)
            return err = "array size inconsistent with its stored bytes", false;
          std::vector<unsigned char> raw(static_cast<size_t>(need), 0);
          if (enc == 1) {
            uLongf len = uLongf(raw.size());
            if (uncompress(raw.data(), &len, &d[o], clen) != Z_OK || len != raw.size()) return err = "bad deflate stream in array", false;
          } else {
            if (clen != raw.size()) return err = "array length mismatch", false;
            memcpy(raw.data(), &d[o], raw.size());
          }
          o += clen;
          p.arr.resize(n);
          for (uint32_t k = 0; k < n; ++k) {
            unsigned char const* q = &raw[size_t(k) * esz];
            if (p.type == 'f') { float v; memcpy(&v, q, 4); p.arr[k] = v; }
            else if (p.type == 'd') { double v; memcpy(&v, q, 8); p.arr[k] = v; }
            else if (p.type == 'i') { int32_t v; memcpy(&v, q, 4); p.arr[k] = v; }
            else if (p.type == 'l') { int64_t v; memcpy(&v, q, 8); p.arr[k] = double(v); }
            else p.arr[k] = q[0];
          }
          break;
        }
        default: return err = std::string("unknown property type '") + p.type + "'", false;
      }
      out.push_back(std::move(p));
    }
    return true;
  }
  // returns 0 on the null record, else the end offset; fills `n`
  bool readNode(size_t o, Node& n, size_t& end, int depth, size_t parentEnd) {
    if (depth > 64) return err = "nesting too deep", false;
    uint64_t e = 0, np = 0, pl = 0;
    size_t hdr;
    if (wide) {
      uint64_t a, b, c;
      if (!get(o, a) || !get(o + 8, b) || !get(o + 16, c)) return false;
      e = a, np = b, pl = c, hdr = 24;
    } else {
      uint32_t a, b, c;
      if (!get(o, a) || !get(o + 4, b) || !get(o + 8, c)) return false;
      e = a, np = b, pl = c, hdr = 12;
    }
    if (e == 0) return end = 0, true;
    if (e > d.size() || e <= o || e > parentEnd) return err = "bad record end offset", false;
    uint8_t nl;
    if (!get(o + hdr, nl)) return false;
    size_t p = o + hdr + 1;
    if (p + nl > d.size()) return err = "truncated name", false;
    n.name.assign(reinterpret_cast<char const*>(&d[p]), nl);
    p += nl;
    size_t const propsEnd = p + size_t(pl);
    if (propsEnd > e) return err = "property list overruns record", false;
    if (!readProps(p, np, n.props)) return false;
    p = propsEnd;
    while (p < e) {
      Node c;
      size_t ce = 0;
      if (!readNode(p, c, ce, depth + 1, size_t(e))) return false;
      if (ce == 0) break;  // null record
      n.children.push_back(std::move(c));
      p = ce;
    }
    end = size_t(e);
    return true;
  }
};

// Properties70/P "name": numeric values after the four descriptor strings
bool prop70(Node const& owner, char const* name, double* out, int n) {
  Node const* p70 = owner.child("Properties70");
  if (!p70) return false;
  for (auto const& P : p70->children) {
    if (P.name != "P" || P.props.empty() || P.props[0].str != name) continue;
    if (int(P.props.size()) < 4 + n) return false;
    for (int i = 0; i < n; ++i) out[i] = P.props[size_t(4 + i)].num;
    return true;
  }
  return false;
}

}  // namespace

static bool readFbxMeshImpl(std::string const& path, std::vector<Triangle>& out, std::string* error, std::vector<float>* uv6,
                            std::vector<float>* n9) {
  auto bad = [&](std::string const& m) {
    if (error) *error = path + ": " + m;
    return false;
  };
  std::ifstream f(path, std::ios::binary);
  if (!f) return bad("cannot open");
  Reader r;
  r.d.assign((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  static char const magic[] = "Kaydara FBX Binary  ";
  if (r.d.size() < 27 || memcmp(r.d.data(), magic, 20) != 0) return bad("not a binary FBX file (ASCII FBX is not supported)");
  uint32_t version;
  memcpy(&version, &r.d[23], 4);
  r.wide = version >= 7500;
  Node root;
  for (size_t o = 27; o + (r.wide ? 25 : 13) <= r.d.size();) {
    Node n;
    size_t end = 0;
    if (!r.readNode(o, n, end, 0, r.d.size())) return bad(r.err);
    if (end == 0) break;
    root.children.push_back(std::move(n));
    o = end;
  }
  Node const* objects = root.child("Objects");
  if (!objects) return bad("no Objects section");
  Node const* geom = nullptr;
  for (auto const& c : objects->children)
    if (c.name == "Geometry" && c.props.size() >= 3 && c.props[2].str == "Mesh" && c.child("Vertices") && c.child("PolygonVertexIndex")) {
      geom = &c;
      break;  // "Only first mesh of this FBX file will be read" (core-mesh-parser.cpp:661-666)
    }
  if (!geom) return bad("No meshes to import");
  std::vector<double> const& V = geom->child("Vertices")->props.empty() ? std::vector<double>() : geom->child("Vertices")->props[0].arr;
  std::vector<double> const& I = geom->child("PolygonVertexIndex")->props.empty() ? std::vector<double>() : geom->child("PolygonVertexIndex")->props[0].arr;
  if (V.empty() || V.size() % 3 || I.empty()) return bad("empty or malformed mesh arrays");

  // the Model this geometry is connected to (Connections: C "OO" child parent)
  double T[3] = {0, 0, 0}, R[3] = {0, 0, 0}, S[3] = {1, 1, 1};
  {
    int64_t const gid = geom->props.empty() ? 0 : int64_t(geom->props[0].num);
    int64_t modelId = 0;
    if (Node const* con = root.child("Connections"))
      for (auto const& c : con->children)
        if (c.name == "C" && c.props.size() >= 3 && c.props[0].str == "OO" && int64_t(c.props[1].num) == gid) modelId = int64_t(c.props[2].num);
    for (auto const& c : objects->children)
      if (c.name == "Model" && !c.props.empty() && int64_t(c.props[0].num) == modelId && modelId != 0) {
        prop70(c, "Lcl Translation", T, 3);
        prop70(c, "Lcl Rotation", R, 3);
        prop70(c, "Lcl Scaling", S, 3);
      }
  }
  double unit = 1.0;  // centimetres per file unit
  if (Node const* gs = root.child("GlobalSettings")) prop70(*gs, "UnitScaleFactor", &unit, 1);
  // M = T * Rz * Ry * Rx * S (FBX eEulerXYZ: X applied first), then the unit scale
  double const kDeg = 3.14159265358979323846 / 180.0;
  double const cx = std::cos(R[0] * kDeg), sx = std::sin(R[0] * kDeg), cy = std::cos(R[1] * kDeg), sy = std::sin(R[1] * kDeg);
  double const cz = std::cos(R[2] * kDeg), sz = std::sin(R[2] * kDeg);
  double const M[3][3] = {{cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx},
                          {sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx},
                          {-sy, cy * sx, cy * cx}};
  // axis system of the file -> (Z up, +Y front, +X coord, left-handed): rows of A are the file's coord, front and up vectors
  double A[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  bool mirrored = false;
  if (Node const* gs = root.child("GlobalSettings")) {
    double up = -1, upS = 1, fr = -1, frS = 1, co = -1, coS = 1;
    bool const have = prop70(*gs, "UpAxis", &up, 1) && prop70(*gs, "FrontAxis", &fr, 1) && prop70(*gs, "CoordAxis", &co, 1);
    prop70(*gs, "UpAxisSign", &upS, 1), prop70(*gs, "FrontAxisSign", &frS, 1), prop70(*gs, "CoordAxisSign", &coS, 1);
    char const* const off = std::getenv("DMT_FBX_AXIS");  // diagnostic knob: DMT_FBX_AXIS=off reads the file's coordinates as they are
    if (have && !(off && std::string(off) == "off")) {
      int const iu = int(up), ifr = int(fr), ic = int(co);
      if (iu < 0 || iu > 2 || ifr < 0 || ifr > 2 || ic < 0 || ic > 2 || iu == ifr || iu == ic || ifr == ic)
        return bad("GlobalSettings: UpAxis / FrontAxis / CoordAxis are not a permutation of the three axes");
      for (auto& row : A) row[0] = row[1] = row[2] = 0;
      A[0][ic] = coS < 0 ? -1 : 1, A[1][ifr] = frS < 0 ? -1 : 1, A[2][iu] = upS < 0 ? -1 : 1;
      double const det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                         A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
      mirrored = det < 0;  // rows (coord, front, up): det = -det[coord up front], negative for a right-handed file
    }
  }
  size_t const nv = V.size() / 3;
  std::vector<Vec3> P(nv);
  for (size_t i = 0; i < nv; ++i) {
    double const x = V[3 * i] * S[0], y = V[3 * i + 1] * S[1], z = V[3 * i + 2] * S[2];
    double const g[3] = {(M[0][0] * x + M[0][1] * y + M[0][2] * z + T[0]) * unit, (M[1][0] * x + M[1][1] * y + M[1][2] * z + T[1]) * unit,
                         (M[2][0] * x + M[2][1] * y + M[2][2] * z + T[2]) * unit};  // the node's global transform, centimetres
    P[i] = Vec3{float(A[0][0] * g[0] + A[0][1] * g[1] + A[0][2] * g[2]), float(A[1][0] * g[0] + A[1][1] * g[1] + A[1][2] * g[2]),
                float(A[2][0] * g[0] + A[2][1] * g[1] + A[2][2] * g[2])};
  }
  // first LayerElementUV (what processUVLayerElement of core-mesh-parser.cpp reads): per polygon vertex ("ByPolygonVertex"),
  // direct or through UVIndex; other mappings (by control point) are resolved through the vertex index
  std::vector<double> const* UV = nullptr;
  std::vector<double> const* UVI = nullptr;
  bool uvByPolygonVertex = true;
  if (Node const* le = geom->child("LayerElementUV")) {
    if (Node const* a = le->child("UV"))
      if (!a->props.empty()) UV = &a->props[0].arr;
    if (Node const* a = le->child("UVIndex"))
      if (!a->props.empty() && !a->props[0].arr.empty()) UVI = &a->props[0].arr;
    if (Node const* a = le->child("MappingInformationType"))
      if (!a->props.empty()) uvByPolygonVertex = a->props[0].str == "ByPolygonVertex";
  }
  auto cornerUv = [&](size_t corner, uint32_t vertex, float* uv) {  // corner = running index over PolygonVertexIndex
    uv[0] = uv[1] = 0.f;
    if (!UV || UV->empty()) return;
    size_t const k = uvByPolygonVertex ? corner : size_t(vertex);
    int64_t idx = UVI ? (k < UVI->size() ? int64_t((*UVI)[k]) : -1) : int64_t(k);
    if (idx < 0 || size_t(2 * idx + 1) >= UV->size()) return;
    uv[0] = float((*UV)[size_t(2 * idx)]), uv[1] = float((*UV)[size_t(2 * idx + 1)]);
  };
  // first LayerElementNormal (the reference's importer insists on one, core-mesh-parser.cpp:448-470): per polygon vertex or
  // by control point, direct or through NormalsIndex, resolved as cornerUv resolves UVs.  A normal transforms by the inverse
  // transpose of the 3x3 that transforms positions, A M S without the translation and the unit scale: A (a signed
  // permutation) and M (a rotation) are their own inverse transposes, so it is A M S^-1; then normalised.
  std::vector<double> const* NR = nullptr;
  std::vector<double> const* NRI = nullptr;
  bool nrByPolygonVertex = true, nrMappingKnown = true;
  if (Node const* le = geom->child("LayerElementNormal")) {
    if (Node const* a = le->child("Normals"))
      if (!a->props.empty()) NR = &a->props[0].arr;
    if (Node const* a = le->child("NormalsIndex"))
      if (!a->props.empty() && !a->props[0].arr.empty()) NRI = &a->props[0].arr;
    if (Node const* a = le->child("MappingInformationType"))
      if (!a->props.empty()) {  // by polygon vertex or by control point; any other mapping (ByPolygon, AllSame, ...) is not read: flat
        std::string const& mt = a->props[0].str;
        nrByPolygonVertex = mt == "ByPolygonVertex";
        nrMappingKnown = nrByPolygonVertex || mt == "ByVertice" || mt == "ByVertex";
      }
    if (Node const* a = le->child("ReferenceInformationType"))
      if (!a->props.empty() && a->props[0].str == "Direct") NRI = nullptr;
  }
  bool const haveNormals = n9 && NR && !NR->empty() && nrMappingKnown;
  auto cornerNormal = [&](size_t corner, uint32_t vertex, float* n) {
    n[0] = n[1] = n[2] = 0.f;
    size_t const k = nrByPolygonVertex ? corner : size_t(vertex);
    int64_t const idx = NRI ? (k < NRI->size() ? int64_t((*NRI)[k]) : -1) : int64_t(k);
    if (idx < 0 || size_t(3 * idx + 2) >= NR->size()) return;
    double const x = S[0] != 0 ? (*NR)[size_t(3 * idx)] / S[0] : 0, y = S[1] != 0 ? (*NR)[size_t(3 * idx + 1)] / S[1] : 0,
                 z = S[2] != 0 ? (*NR)[size_t(3 * idx + 2)] / S[2] : 0;
    double const g[3] = {M[0][0] * x + M[0][1] * y + M[0][2] * z, M[1][0] * x + M[1][1] * y + M[1][2] * z, M[2][0] * x + M[2][1] * y + M[2][2] * z};
    double const w[3] = {A[0][0] * g[0] + A[0][1] * g[1] + A[0][2] * g[2], A[1][0] * g[0] + A[1][1] * g[1] + A[1][2] * g[2],
                         A[2][0] * g[0] + A[2][1] * g[1] + A[2][2] * g[2]};
    double const len = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    if (!(len > 0) || !std::isfinite(len)) return;
    n[0] = float(w[0] / len), n[1] = float(w[1] / len), n[2] = float(w[2] / len);
  };
  out.clear();
  if (uv6) uv6->clear();
  if (n9) n9->clear();
  std::vector<uint32_t> poly;
  std::vector<size_t> polyCorner;
  size_t corner = 0;
  for (double di : I) {
    int64_t idx = int64_t(di);
    bool const last = idx < 0;
    if (last) idx = ~idx;  // the last index of a polygon is stored as its bitwise complement
    if (idx < 0 || size_t(idx) >= nv) return bad("vertex index out of range");
    poly.push_back(uint32_t(idx));
    polyCorner.push_back(corner++);
    if (last) {
      for (size_t k = 1; k + 1 < poly.size(); ++k) {
        size_t const b = mirrored ? k + 1 : k, c = mirrored ? k : k + 1;  // a reflection reverses the winding
        out.push_back(Triangle{P[poly[0]], P[poly[b]], P[poly[c]]});
        if (uv6) {
          float uv[6];
          cornerUv(polyCorner[0], poly[0], uv), cornerUv(polyCorner[b], poly[b], uv + 2), cornerUv(polyCorner[c], poly[c], uv + 4);
          uv6->insert(uv6->end(), uv, uv + 6);
        }
        if (haveNormals) {  // the corners the triangle was made of, in its (possibly reversed) order
          float nn[9];
          cornerNormal(polyCorner[0], poly[0], nn), cornerNormal(polyCorner[b], poly[b], nn + 3), cornerNormal(polyCorner[c], poly[c], nn + 6);
          for (int v = 0; v < 3; ++v)  // a corner without a usable normal: the whole triangle stays flat (nine zeros)
            if (nn[3 * v] == 0.f && nn[3 * v + 1] == 0.f && nn[3 * v + 2] == 0.f) std::fill(nn, nn + 9, 0.f);
          n9->insert(n9->end(), nn, nn + 9);
        }
      }
      poly.clear(), polyCorner.clear();
    }
  }
  if (out.empty()) return bad("mesh has no polygons");
  return true;
}

// Files are untrusted input: nothing escapes as an exception (allocation failure on a forged size, ...).
bool readFbxMesh(std::string const& path, std::vector<Triangle>& out, std::string* error, std::vector<float>* uv6, std::vector<float>* n9) {
  try {
    return readFbxMeshImpl(path, out, error, uv6, n9);
  } catch (std::exception const& e) {
    if (error) *error = path + ": " + e.what();
  } catch (...) {
    if (error) *error = path + ": unknown error";
  }
  out.clear();
  if (n9) n9->clear();
  return false;
}

}  // namespace dmt_host
