// dmt-megakernel-hip -- command-line driver with the reference's two CLI surfaces:
//   * dmt-megakernel (examples/triangles/megakernel/main.cu:67-243; flags CC/private/host_utils.cu:39-92):
//       --width <N> --height <N> --spp <N> --kspp <N> --log-level info|verbose --save-partial
//   * dmt-tracer (cli/CLIManager.cpp:11-36): --device|-d cpu|gpu, --scene|-s <file>, --out|-o <path>, --time|-t,
//       --help|-h.  `--device cpu` is refused: this build has no CPU renderer (the CPU restatement used by the tests is test
//       infrastructure and is never linked into the product).
// plus --max-depth <N> (reference constant 32), --gpu-ordinal <N>, --bvh, --bvh-build host|gpu, --light-tree, --light-tree-reference, --emitter-tree, --texture-filter,
// --adaptive <threshold> / --min-spp <N> (dmt_render_adaptive: --spp is the cap, --kspp the round), and --gpus <N>: N contexts, one per GPU
// (ordinals 0..N-1), each rendering the interleaved 8x8 tiles j mod N == rank (dmt_set_partition) concurrently; the N
// films are disjoint and summed on the host (x + 0: an exact gather).  bench.py's N-process RCCL path is the scalable
// form of the same partition; --gpus is the single-process form for the CLI.
// Renders the hard-coded cornellBox() scene (or --scene) kspp samples per launch and writes
// output-<spp>.png and output-<spp>_sqrt_mse.png next to the executable (or into --out).
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "dmt_scene.hpp"

namespace {

struct Config {  // defaults: CC/public/cuda-core/host_utils.cuh:25-31
  int width = 256, height = 256, spp = 2048, kspp = 4;
  int maxDepth = 32, device = 0, gpus = 1;
  std::string deviceKind = "gpu";  // cli/CLIManager.cpp:12-16 (the reference's default is cpu; this build only has gpu)
  bool timeReport = false;         // --time / -t
  bool bad = false;                // unknown option / missing value
  std::string badWhat;
  std::string logLevel = "info", outDir;
  bool savePartial = false;
  std::string scenePath;  // --scene <file.json>: the reference's JSON scene description instead of cornellBox()
  bool bvh = false;       // --bvh: traverse the 4-wide BVH instead of testing every triangle
  bool lightTree = false; // --light-tree: importance-driven light choice (csrc/light_tree.hpp) instead of the uniform pick
  bool textureFilter = false; // --texture-filter: first-hit MIP / EWA filtering of image textures (DMT_TEXFILTER_REFERENCE)
  bool emitterTree = false; // --emitter-tree: emissive triangles and lights picked through the emitter tree (csrc/emitter_tree.hpp)
  bool lightTreeRef = false; // --light-tree-reference: the reference's tree semantics, up to four lights per bounce (csrc/light_tree_ref.hpp)
  bool widthSet = false, heightSet = false, sppSet = false, depthSet = false;
  bool adaptive = false;      // --adaptive <threshold>: adaptive sampling, --spp samples at most, rounds of --kspp
  std::string adaptiveArg;
  float threshold = 0.f;      // parsed from adaptiveArg by validate()
  int minSpp = 0;             // --min-spp <N>: samples every pixel gets before the stopping rule applies
  bool minSppSet = false;
  bool denoise = false;       // --denoise: also write output-<spp>_denoised.png (dmt_render_aovs + dmt_denoise)
  int aovSpp = 4;             // --aov-spp <N>: camera samples per pixel of the feature buffers
  bool aovSppSet = false;
  bool lensRadiusSet = false, focusDistanceSet = false, focusPixelSet = false;  // --lens-radius R, --focus-distance D, --focus-pixel X Y
  float lensRadius = 0.f, focusDistance = 1.f, focusX = 0.f, focusY = 0.f;
  // --pixel-filter box|tent|gaussian|blackman-harris|scene, --filter-radius R, --filter-sigma S (dmt_set_pixel_filter)
  std::string pixelFilter;
  std::string projection;     // --projection perspective|orthographic|equirect|fisheye (dmt_set_projection); empty: the scene file's
  bool orthoHeightSet = false, fisheyeFovSet = false;  // --ortho-height H, --fisheye-fov DEG
  float orthoHeight = 0.f, fisheyeFov = 0.f;
  bool filterRadiusSet = false, filterSigmaSet = false;
  float filterRadius = 0.f, filterSigma = 0.5f;
  bool shutterSet = false;    // --shutter OPEN CLOSE: the shutter interval of --motion-scene (dmt_set_shutter)
  float shutterOpen = 0.f, shutterClose = 1.f;
  std::string motionScenePath;  // --motion-scene <file>: the same scene at the end of the frame; its triangle positions become key 1
  std::string shadingNormals = "off";  // --shading-normals off|file|smooth[:DEG] (dmt_upload_vertex_normals)
  float creaseDegrees = 180.f;         // parsed from shadingNormals by validate()
  std::string cutouts = "on";  // --cutouts on|off: upload the scene's opacity textures (dmt_upload_opacity), or ignore them
  // --medium SIGMA_T [--medium-albedo R G B] [--medium-g G] [--medium-box X0 Y0 Z0 X1 Y1 Z1]: homogeneous fog (dmt_set_medium)
  bool mediumSet = false, mediumAlbedoSet = false, mediumGSet = false, mediumBoxSet = false;
  float mediumSigmaT = 0.f, mediumG = 0.f, mediumAlbedo[3] = {1.f, 1.f, 1.f}, mediumBox[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  // --medium-extinction R G B, --medium-emission R G B: its spectrum (dmt_set_medium_spectrum)
  bool mediumExtinctionSet = false, mediumEmissionSet = false;
  float mediumExtinction[3] = {1.f, 1.f, 1.f}, mediumEmission[3] = {0.f, 0.f, 0.f};
  std::string mediumGridPath;  // --medium-grid FILE: a density grid for the medium (dmt_set_medium_grid), a NumPy .npy file
  bool bvhBuildSet = false;   // --bvh-build host|gpu: who builds the tree of --bvh (dmt_set_accel_build)
  std::string bvhBuildArg;
  // the display transform (dmt_display): any of these also writes output-<spp>_display.png.  --tonemap, --exposure EV|auto,
  // --exposure-key K, --white W, --bloom S, --bloom-levels K, --oetf, --dither
  bool display = false;
  std::string tonemap = "aces", exposure = "0", oetf = "srgb";
  bool exposureKeySet = false, whiteSet = false, bloomSet = false, bloomLevelsSet = false, dither = false;
  float exposureKey = 0.18f, white = 0.f, bloom = 0.f;
  int bloomLevels = 5;        // the levels of --bloom unless --bloom-levels says otherwise
  bool hdr = false;           // --hdr: also write output-<spp>.pfm, the linear mean

  // --shading-normals' value: off, file, smooth or smooth:DEG with 0 <= DEG <= 180
  static bool parseShadingNormals(std::string const& a, float& crease) {
    if (a == "off" || a == "file" || a == "smooth") return true;
    if (a.compare(0, 7, "smooth:") != 0) return false;
    char* end = nullptr;
    float const v = std::strtof(a.c_str() + 7, &end);
    if (a.size() == 7 || end != a.c_str() + a.size() || !std::isfinite(v) || v < 0.f || v > 180.f) return false;
    crease = v;
    return true;
  }
  // --adaptive's value: a finite, non-negative number and nothing else
  static bool parseThreshold(std::string const& a, float& out) {
    char* end = nullptr;
    float const v = std::strtof(a.c_str(), &end);
    if (a.empty() || end != a.c_str() + a.size() || !std::isfinite(v) || v < 0.f) return false;
    out = v;
    return true;
  }

  std::string validate() const {  // host_utils.cuh:35-62
    if (width <= 0) return "invalid width: should be bigger than zero. got " + std::to_string(width);
    if (height <= 0) return "invalid height: should be bigger than zero. got " + std::to_string(height);
    if (spp <= 0) return "invalid spp: should be bigger than zero. got " + std::to_string(spp);
    if (spp < kspp) return "invalid spp: should be bigger than kspp. got " + std::to_string(spp) + " and kspp" + std::to_string(kspp);
    if (kspp <= 0) return "invalid kspp: should be bigger than zero. got " + std::to_string(kspp);
    if (logLevel != "info" && logLevel != "verbose") return "invalid logLevel value. Either info or verbose, got " + logLevel;
    if (maxDepth < 0) return "invalid max-depth";
    if (bad) return badWhat;
    if (deviceKind != "cpu" && deviceKind != "gpu") return "--device: wrong argument is not allowed. (cpu or gpu, got " + deviceKind + ")";
    if (gpus < 1 || gpus > 64) return "invalid --gpus: expected 1..64, got " + std::to_string(gpus);
    if (device < 0) return "invalid --gpu-ordinal";
    if (minSppSet && !adaptive) return "--min-spp needs --adaptive";
    if (adaptive) {
      float t = 0.f;
      if (!parseThreshold(adaptiveArg, t)) return "invalid --adaptive: expected a finite threshold >= 0, got '" + adaptiveArg + "'";
      if (minSpp < 0) return "invalid --min-spp: should not be negative. got " + std::to_string(minSpp);
      if (minSpp > spp) return "invalid --min-spp: should not exceed spp. got " + std::to_string(minSpp) + " and spp " + std::to_string(spp);
      if (spp > (1 << 24)) return "invalid spp: --adaptive allows at most 2^24 samples per pixel";
      if (savePartial) return "--save-partial is not available with --adaptive";
    }
    if (aovSppSet && !denoise) return "--aov-spp needs --denoise";
    if (bvhBuildSet && bvhBuildArg != "host" && bvhBuildArg != "gpu") return "invalid --bvh-build: expected host or gpu, got '" + bvhBuildArg + "'";
    if (bvhBuildSet && !bvh) return "--bvh-build needs --bvh";
    if (lensRadiusSet && !(std::isfinite(lensRadius) && lensRadius >= 0.f)) return "invalid --lens-radius: expected a finite radius >= 0";
    if (focusDistanceSet && !(std::isfinite(focusDistance) && focusDistance > 0.f)) return "invalid --focus-distance: expected a finite distance > 0";
    if (focusDistanceSet && focusPixelSet) return "--focus-distance and --focus-pixel exclude each other";
    if (focusPixelSet && !(focusX >= 0.f && focusX < float(width) && focusY >= 0.f && focusY < float(height))) return "invalid --focus-pixel: outside the frame";
    if (!projection.empty() && projection != "perspective" && projection != "orthographic" && projection != "equirect" && projection != "fisheye")
      return "invalid --projection: expected perspective, orthographic, equirect or fisheye, got '" + projection + "'";
    if (orthoHeightSet != (projection == "orthographic")) return "--ortho-height goes with --projection orthographic, and only with it";
    if (fisheyeFovSet != (projection == "fisheye")) return "--fisheye-fov goes with --projection fisheye, and only with it";
    if (orthoHeightSet && !(std::isfinite(orthoHeight) && orthoHeight > 0.f)) return "invalid --ortho-height: expected a finite height > 0";
    if (fisheyeFovSet && !(fisheyeFov > 0.f && fisheyeFov <= 360.f)) return "invalid --fisheye-fov: expected degrees in (0, 360]";
    if (!pixelFilter.empty() && pixelFilter != "box" && pixelFilter != "tent" && pixelFilter != "gaussian" && pixelFilter != "blackman-harris" &&
        pixelFilter != "scene")
      return "invalid --pixel-filter: expected box, tent, gaussian, blackman-harris or scene, got '" + pixelFilter + "'";
    if ((filterRadiusSet || filterSigmaSet) && (pixelFilter.empty() || pixelFilter == "scene")) return "--filter-radius and --filter-sigma need --pixel-filter with a kind";
    if (filterRadiusSet && !(std::isfinite(filterRadius) && filterRadius > 0.f && filterRadius <= 8.f)) return "invalid --filter-radius: expected a radius in (0, 8] pixels";
    if (filterSigmaSet && pixelFilter != "gaussian") return "--filter-sigma needs --pixel-filter gaussian";
    if (filterSigmaSet && !(std::isfinite(filterSigma) && filterSigma > 0.f)) return "invalid --filter-sigma: expected a finite sigma > 0";
    if (shutterSet && !(std::isfinite(shutterOpen) && std::isfinite(shutterClose) && 0.f <= shutterOpen && shutterOpen <= shutterClose && shutterClose <= 1.f))
      return "invalid --shutter: expected 0 <= OPEN <= CLOSE <= 1";
    if (float c = 180.f; !parseShadingNormals(shadingNormals, c))
      return "invalid --shading-normals: expected off, file, smooth or smooth:DEG (0 <= DEG <= 180), got '" + shadingNormals + "'";
    if (shadingNormals != "off" && !motionScenePath.empty()) return "--shading-normals and --motion-scene exclude each other";
    if (cutouts != "on" && cutouts != "off") return "invalid --cutouts: expected on or off, got '" + cutouts + "'";
    if ((mediumAlbedoSet || mediumGSet || mediumBoxSet) && !mediumSet) return "--medium-albedo, --medium-g and --medium-box need --medium";
    if ((mediumExtinctionSet || mediumEmissionSet) && !mediumSet) return "--medium-extinction and --medium-emission need --medium";
    if (mediumExtinctionSet) {
      for (float v : mediumExtinction)
        if (!(std::isfinite(v) && v >= 0.f)) return "invalid --medium-extinction: expected three finite numbers >= 0, not all zero";
      if (mediumExtinction[0] == 0.f && mediumExtinction[1] == 0.f && mediumExtinction[2] == 0.f)
        return "invalid --medium-extinction: expected three finite numbers >= 0, not all zero";
    }
    if (mediumEmissionSet)
      for (float v : mediumEmission)
        if (!(std::isfinite(v) && v >= 0.f)) return "invalid --medium-emission: expected three finite numbers >= 0";
    if (mediumSet && !(std::isfinite(mediumSigmaT) && mediumSigmaT >= 0.f)) return "invalid --medium: expected a finite extinction coefficient >= 0";
    if (mediumAlbedoSet && !(mediumAlbedo[0] >= 0.f && mediumAlbedo[0] <= 1.f && mediumAlbedo[1] >= 0.f && mediumAlbedo[1] <= 1.f && mediumAlbedo[2] >= 0.f && mediumAlbedo[2] <= 1.f))
      return "invalid --medium-albedo: expected three numbers in [0, 1]";
    if (mediumGSet && !(std::fabs(mediumG) < 1.f)) return "invalid --medium-g: expected a number in (-1, 1)";
    if (mediumBoxSet)
      for (int i = 0; i < 3; ++i)
        if (!(std::isfinite(mediumBox[i]) && std::isfinite(mediumBox[3 + i]) && mediumBox[i] < mediumBox[3 + i]))
          return "invalid --medium-box: expected finite X0 Y0 Z0 X1 Y1 Z1 with X0 < X1, Y0 < Y1, Z0 < Z1";
    if (!mediumGridPath.empty() && mediumSet && !(mediumSigmaT > 0.f)) return "--medium-grid needs a medium: --medium 0 switches it off";
    if (mediumSet && mediumSigmaT > 0.f && denoise) return "--medium and --denoise exclude each other (the feature buffers do not know the fog)";
    if (aovSpp < 1 || aovSpp > 65536) return "invalid --aov-spp: expected 1..65536, got " + std::to_string(aovSpp);
    if (tonemap != "linear" && tonemap != "reinhard" && tonemap != "aces" && tonemap != "hable")
      return "invalid --tonemap: expected linear, reinhard, aces or hable, got '" + tonemap + "'";
    if (oetf != "linear" && oetf != "srgb" && oetf != "gamma22") return "invalid --oetf: expected linear, srgb or gamma22, got '" + oetf + "'";
    if (float ev = 0.f; exposure != "auto" && !parseNumber(exposure, ev)) return "invalid --exposure: expected a finite EV or auto, got '" + exposure + "'";
    if (exposureKeySet && exposure != "auto") return "--exposure-key needs --exposure auto";
    if (exposureKeySet && !(std::isfinite(exposureKey) && exposureKey > 0.f)) return "invalid --exposure-key: expected a finite key > 0";
    if (whiteSet && !(std::isfinite(white) && white > 0.f)) return "invalid --white: expected a finite white point > 0";
    if (whiteSet && tonemap != "reinhard" && tonemap != "hable") return "--white needs --tonemap reinhard or hable";
    if (bloomSet && !(bloom >= 0.f && bloom <= 1.f)) return "invalid --bloom: expected a strength in [0, 1]";
    if (bloomLevelsSet && !bloomSet) return "--bloom-levels needs --bloom";
    if (bloomLevelsSet && (bloomLevels < 0 || bloomLevels > 8)) return "invalid --bloom-levels: expected 0..8, got " + std::to_string(bloomLevels);
    return "";
  }
  // a finite number and nothing else
  static bool parseNumber(std::string const& a, float& out) {
    char* end = nullptr;
    float const v = std::strtof(a.c_str(), &end);
    if (a.empty() || end != a.c_str() + a.size() || !std::isfinite(v)) return false;
    out = v;
    return true;
  }
  // the parameters of the flags, over dmt_display_defaults()
  dmt_display_params displayParams() const {
    dmt_display_params p = dmt_display_defaults();
    p.tone = tonemap == "linear" ? DMT_TONE_LINEAR : tonemap == "reinhard" ? DMT_TONE_REINHARD : tonemap == "hable" ? DMT_TONE_HABLE : DMT_TONE_ACES;
    p.oetf = oetf == "linear" ? DMT_OETF_LINEAR : oetf == "gamma22" ? DMT_OETF_GAMMA22 : DMT_OETF_SRGB;
    p.auto_exposure = exposure == "auto" ? 1 : 0;
    if (!p.auto_exposure) parseNumber(exposure, p.exposure_ev);
    if (exposureKeySet) p.key = exposureKey;
    if (whiteSet) p.white = white;
    if (bloomSet) p.bloom_strength = bloom, p.bloom_levels = bloomLevels;
    if (dither) p.quantiser = DMT_QUANT_DITHER;
    return p;
  }
};

void printHelp() {
  std::puts(
      "Input Commands:\n"
      "  --width <N>       -- Define Width of output image\n"
      "  --height <N>      -- Define Height of output image\n"
      "  --spp <N>         -- Define Samples per pixel\n"
      "  --kspp <N>        -- Define Samples per pixel processed on a single kernel loop\n"
      "  --log-level <N>   -- Log Verbosity, 'info' or 'verbose'\n"
      "  --save-partial    -- Whether to save images every <kspp> samples\n"
      "  --max-depth <N>   -- Bounce cap (reference: 32)\n"
      "  --device, -d <cpu|gpu> -- Device used for the rendering (only gpu is built; cpu is refused)\n"
      "  --gpu-ordinal <N> -- First GPU ordinal (default 0)\n"
      "  --gpus <N>        -- Partition the frame over N GPUs (ordinals gpu-ordinal .. +N-1), interleaved 8x8 tiles\n"
      "  --time, -t        -- Measure and report the execution times of key rendering operations\n"
      "  --out, -o <dir>   -- Output directory (default: the executable's directory)\n"
      "  --help, -h        -- This text\n"
      "  --scene, -s <file> -- JSON scene (camera/film/materials/objects/lights/envlight/transforms/world) or *.pbrt\n"
      "                       (PBRT-v4 subset: diffuse materials, triangle meshes, diffuse area lights);\n"
      "                       its resolution, samples and max-depth apply unless given on the command line\n"
      "  --bvh             -- BVH traversal instead of the brute-force triangle loop\n"
      "  --bvh-build <host|gpu> -- who builds the tree of --bvh: one host core (binned SAH, the default) or the GPU (LBVH:\n"
      "                       a much faster build of a slightly looser tree; same image bit for bit)\n"
      "  --light-tree      -- pick the NEE light through a light BVH (flux x cosine / distance^2) instead of uniformly\n"
      "  --emitter-tree    -- with emissive triangles: pick the NEE emitter (triangle or light) through a light BVH with normal\n"
      "                       cones instead of uniformly; without emissive triangles it changes nothing\n"
      "  --light-tree-reference -- the reference's light tree semantics: cones, adaptive cuts, up to four lights per bounce\n"
      "  --texture-filter  -- filter image textures at the camera ray's first hit (MIP levels / EWA by the pixel footprint)\n"
      "                       instead of the level-0 bilinear lookup\n"
      "  --adaptive <T>    -- Adaptive sampling: rounds of --kspp samples; a pixel stops at --spp samples, or once it has\n"
      "                       --min-spp and the relative standard error of its mean is <= T.  Also writes\n"
      "                       output-<spp>_spp.png, the samples each pixel received / spp\n"
      "  --min-spp <N>     -- Samples every pixel receives before --adaptive may stop it (default 0)\n"
      "  --denoise         -- Also write output-<spp>_denoised.png: the film through an a-trous filter guided by its variance\n"
      "                       and first-hit albedo / normal / position buffers (every other output stays as without it)\n"
      "  --aov-spp <N>     -- Camera samples per pixel of those buffers (default 4)\n"
      "  --lens-radius <R> -- Thin lens of radius R in scene units: depth of field (0, the default, is the pinhole; a scene\n"
      "                       file's own lens applies unless given here)\n"
      "  --projection <P>  -- Camera projection: perspective (the default), orthographic (with --ortho-height), equirect (a\n"
      "                       360-degree panorama; 2:1 frames are the natural shape) or fisheye (equidistant, with\n"
      "                       --fisheye-fov).  A scene file's own projection applies unless given here.  Not with\n"
      "                       --lens-radius, --denoise or --texture-filter\n"
      "  --ortho-height <H> -- Height of the orthographic view, in scene units\n"
      "  --fisheye-fov <DEG> -- Field of view of the fisheye across the frame's diagonal, in degrees (0, 360]\n"
      "  --focus-distance <D> -- Depth along the viewing direction, in scene units, that the lens renders sharp\n"
      "  --focus-pixel <X> <Y> -- Autofocus: focus on what the centre of pixel (X, Y) shows, and print the distance chosen\n"
      "  --pixel-filter <box|tent|gaussian|blackman-harris|scene> -- Pixel reconstruction filter, importance-sampled per sample\n"
      "                       (every sample keeps weight 1).  Default: the box of radius 0.5, as the reference renders.  scene:\n"
      "                       the filter the scene file records (PBRT PixelFilter, JSON film.filter), which is ignored otherwise\n"
      "  --filter-radius <R> -- Its radius in pixels, in (0, 8] (defaults: box 0.5, tent 2, gaussian 1.5, blackman-harris 2)\n"
      "  --filter-sigma <S> -- The Gaussian's sigma in pixels (default 0.5)\n"
      "  --motion-scene <file> -- Motion blur: a second scene file of the same kind as --scene whose triangle positions are\n"
      "                       where the triangles are at the end of the frame (same triangles, same order); every sample\n"
      "                       sees the scene at its own time in between\n"
      "  --shutter <OPEN> <CLOSE> -- The part of the frame the shutter is open, 0 <= OPEN <= CLOSE <= 1 (default 0 1)\n"
      "  --shading-normals <off|file|smooth[:DEG]> -- Smooth shading: interpolate per-vertex normals at every hit.  off (the\n"
      "                       default): faceted, as the reference renders.  file: the normals of the scene's meshes (FBX normal\n"
      "                       layers, PBRT \"normal N\"); meshes without any stay faceted.  smooth: normals computed from the\n"
      "                       geometry, angle-weighted over the faces that meet at a vertex within DEG degrees of each\n"
      "                       other (default 180: no crease)\n"
      "  --cutouts <on|off> -- Alpha cutouts: a material's \"opacity\" texture decides at every hit whether the hit counts (A\n"
      "                       channel >= the material's \"opacity-cutoff\", default 0.5), for camera, bounce and shadow rays.\n"
      "                       on (the default): as the scene says; scenes without opacity textures are unaffected.  off:\n"
      "                       ignore them, every triangle is solid\n"
      "  --medium <SIGMA_T> -- Participating medium: homogeneous fog of extinction SIGMA_T per scene unit (0: none), sampled\n"
      "                       in-path: light shafts, glow and depth cueing from the scene's own lights.  Overrides the scene\n"
      "                       file's \"medium\"\n"
      "  --medium-albedo <R> <G> <B> -- Its single-scattering albedo per channel, in [0, 1] (default 1 1 1)\n"
      "  --medium-g <G>    -- Its Henyey-Greenstein asymmetry, in (-1, 1): 0 isotropic (the default), > 0 forward\n"
      "  --medium-box <X0> <Y0> <Z0> <X1> <Y1> <Z1> -- The box that holds it (default: the bounds of the scene's triangles)\n"
      "  --medium-extinction <R> <G> <B> -- Its extinction colour: the channel extinctions are SIGMA_T times these (default\n"
      "                       1 1 1, grey); three numbers >= 0, not all zero.  Unequal channels are sampled by one-sample MIS\n"
      "  --medium-emission <R> <G> <B> -- The radiance it emits per channel, >= 0 (default 0 0 0): a glowing gas\n"
      "  --medium-grid <FILE> -- A density grid that fills the medium's box: the extinction in a voxel is SIGMA_T times its\n"
      "                       density, marched exactly.  A NumPy .npy file (version 1.0 or 2.0, little-endian float32, C order,\n"
      "                       shape (nz, ny, nx), values finite and >= 0).  Needs a medium, from --medium or the scene file;\n"
      "                       replaces the scene file's \"grid\"\n"
      "  --tonemap <linear|reinhard|aces|hable> -- Display transform: any of this and the next seven flags also writes\n"
      "                       output-<spp>_display.png (and output-<spp>_denoised_display.png with --denoise): the linear film\n"
      "                       through exposure, bloom, this tone curve (default aces), a transfer function and a rounding\n"
      "                       quantiser, on the GPU.  Every other output stays as without them\n"
      "  --exposure <EV|auto> -- Exposure in stops (default 0), or auto: metered from a histogram of the log luminance so\n"
      "                       that its trimmed average lands on the key\n"
      "  --exposure-key <K> -- The key of --exposure auto (default 0.18)\n"
      "  --white <W>       -- White point of --tonemap reinhard (default 4) or hable (default 11.2)\n"
      "  --bloom <S>       -- Bloom strength in [0, 1] (default 0: none): the frame mixed with a blur pyramid of itself\n"
      "  --bloom-levels <K> -- Levels of that pyramid, 0..8 (default 5)\n"
      "  --oetf <linear|srgb|gamma22> -- Transfer function (default srgb)\n"
      "  --dither          -- Quantise with an 8x8 ordered dither instead of rounding\n"
      "  --hdr             -- Also write output-<spp>.pfm: the linear mean as a little-endian RGB Portable Float Map");
}

Config parseArguments(int argc, char** argv) {
  Config c;
  for (int i = 1; i < argc; ++i) {
    std::string const a = argv[i];
    bool const more = i + 1 < argc;
    if (a == "--width" && more) c.width = std::atoi(argv[++i]), c.widthSet = true;
    else if (a == "--height" && more) c.height = std::atoi(argv[++i]), c.heightSet = true;
    else if (a == "--spp" && more) c.spp = std::atoi(argv[++i]), c.sppSet = true;
    else if ((a == "--scene" || a == "-s") && more) c.scenePath = argv[++i];
    else if (a == "--bvh") c.bvh = true;
    else if (a == "--bvh-build" && more) c.bvhBuildSet = true, c.bvhBuildArg = argv[++i];
    else if (a == "--light-tree") c.lightTree = true;
    else if (a == "--light-tree-reference") c.lightTreeRef = true;
    else if (a == "--emitter-tree") c.emitterTree = true;
    else if (a == "--texture-filter") c.textureFilter = true;
    else if (a == "--kspp" && more) c.kspp = std::atoi(argv[++i]);
    else if (a == "--adaptive" && more) c.adaptive = true, c.adaptiveArg = argv[++i];
    else if (a == "--min-spp" && more) c.minSpp = std::atoi(argv[++i]), c.minSppSet = true;
    else if (a == "--denoise") c.denoise = true;
    else if (a == "--aov-spp" && more) c.aovSpp = std::atoi(argv[++i]), c.aovSppSet = true;
    else if (a == "--lens-radius" && more) c.lensRadius = std::strtof(argv[++i], nullptr), c.lensRadiusSet = true;
    else if (a == "--focus-distance" && more) c.focusDistance = std::strtof(argv[++i], nullptr), c.focusDistanceSet = true;
    else if (a == "--focus-pixel" && i + 2 < argc) c.focusX = std::strtof(argv[++i], nullptr), c.focusY = std::strtof(argv[++i], nullptr), c.focusPixelSet = true;
    else if (a == "--shutter" && i + 2 < argc) c.shutterOpen = std::strtof(argv[++i], nullptr), c.shutterClose = std::strtof(argv[++i], nullptr), c.shutterSet = true;
    else if (a == "--motion-scene" && more) c.motionScenePath = argv[++i];
    else if (a == "--shading-normals" && more) c.shadingNormals = argv[++i];
    else if (a == "--cutouts" && more) c.cutouts = argv[++i];
    else if (a == "--pixel-filter" && more) c.pixelFilter = argv[++i];
    else if (a == "--projection" && more) c.projection = argv[++i];
    else if (a == "--ortho-height" && more) c.orthoHeight = std::strtof(argv[++i], nullptr), c.orthoHeightSet = true;
    else if (a == "--fisheye-fov" && more) c.fisheyeFov = std::strtof(argv[++i], nullptr), c.fisheyeFovSet = true;
    else if (a == "--filter-radius" && more) c.filterRadius = std::strtof(argv[++i], nullptr), c.filterRadiusSet = true;
    else if (a == "--filter-sigma" && more) c.filterSigma = std::strtof(argv[++i], nullptr), c.filterSigmaSet = true;
    else if (a == "--medium" && more) c.mediumSigmaT = std::strtof(argv[++i], nullptr), c.mediumSet = true;
    else if (a == "--medium-grid" && more) c.mediumGridPath = argv[++i];
    else if (a == "--medium-g" && more) c.mediumG = std::strtof(argv[++i], nullptr), c.mediumGSet = true;
    else if (a == "--medium-albedo" && i + 3 < argc) {
      for (float& v : c.mediumAlbedo) v = std::strtof(argv[++i], nullptr);
      c.mediumAlbedoSet = true;
    } else if (a == "--medium-extinction" && i + 3 < argc) {
      for (float& v : c.mediumExtinction) v = std::strtof(argv[++i], nullptr);
      c.mediumExtinctionSet = true;
    } else if (a == "--medium-emission" && i + 3 < argc) {
      for (float& v : c.mediumEmission) v = std::strtof(argv[++i], nullptr);
      c.mediumEmissionSet = true;
    } else if (a == "--medium-box" && i + 6 < argc) {
      for (float& v : c.mediumBox) v = std::strtof(argv[++i], nullptr);
      c.mediumBoxSet = true;
    }
    else if (a == "--tonemap" && more) c.tonemap = argv[++i], c.display = true;
    else if (a == "--exposure" && more) c.exposure = argv[++i], c.display = true;
    else if (a == "--exposure-key" && more) c.exposureKey = std::strtof(argv[++i], nullptr), c.exposureKeySet = c.display = true;
    else if (a == "--white" && more) c.white = std::strtof(argv[++i], nullptr), c.whiteSet = c.display = true;
    else if (a == "--bloom" && more) c.bloom = std::strtof(argv[++i], nullptr), c.bloomSet = c.display = true;
    else if (a == "--bloom-levels" && more) c.bloomLevels = std::atoi(argv[++i]), c.bloomLevelsSet = c.display = true;
    else if (a == "--oetf" && more) c.oetf = argv[++i], c.display = true;
    else if (a == "--dither") c.dither = c.display = true;
    else if (a == "--hdr") c.hdr = true;
    else if (a == "--log-level" && more) c.logLevel = argv[++i];
    else if (a == "--save-partial") c.savePartial = true;
    else if (a == "--max-depth" && more) c.maxDepth = std::atoi(argv[++i]), c.depthSet = true;
    else if ((a == "--device" || a == "-d") && more) c.deviceKind = argv[++i];
    else if (a == "--gpu-ordinal" && more) c.device = std::atoi(argv[++i]);
    else if (a == "--gpus" && more) c.gpus = std::atoi(argv[++i]);
    else if (a == "--time" || a == "-t") c.timeReport = true;
    else if ((a == "--out" || a == "-o") && more) c.outDir = argv[++i];
    else if (a == "--help" || a == "-h") { printHelp(); std::exit(0); }
    else if (!c.bad) c.bad = true, c.badWhat = "Unknown option (or missing value): " + a;  // CLIManager.cpp:52-56
  }
  return c;
}

std::string executableDirectory() {
  char buf[PATH_MAX];
  ssize_t const n = readlink("/proc/self/exe", buf, sizeof(buf) - 1);
  if (n <= 0) return ".";
  buf[n] = 0;
  std::string p(buf);
  size_t const slash = p.find_last_of('/');
  return slash == std::string::npos ? "." : p.substr(0, slash);
}

struct Contexts {  // one dmt_ctx per GPU of the run; destroyed on every exit path
  std::vector<dmt_ctx*> v;
  ~Contexts() {
    for (dmt_ctx* c : v)
      if (c) dmt_ctx_destroy(c);
  }
};

int fail(dmt_ctx* ctx, char const* what) {
  std::fprintf(stderr, "%s failed: %s\n", what, dmt_last_error(ctx));
  return 1;
}

double msSince(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

int main(int argc, char** argv) {
  Config cfg = parseArguments(argc, argv);
  if (cfg.deviceKind == "cpu") {  // the reference's CLI default (CLIManager.cpp:12-16); not part of this build
    std::fprintf(stderr, "--device cpu: not built.  This is the HIP path of the renderer; it has no CPU fallback "
                         "(the CPU restatement used by the tests is not part of the product).  Use --device gpu.\n");
    return 1;
  }
  auto const tLoad = std::chrono::steady_clock::now();
  dmt_host::JsonScene json;
  if (!cfg.scenePath.empty()) {
    std::string err;
    bool const pbrt = cfg.scenePath.size() > 5 && cfg.scenePath.compare(cfg.scenePath.size() - 5, 5, ".pbrt") == 0;
    bool ok;
    if (pbrt) {  // PBRT-v4 subset (scenes/cornell-box.pbrt); same fields as the JSON front-end
      dmt_host::PbrtScene ps;
      ok = dmt_host::loadPbrtScene(cfg.scenePath, ps, &err);
      json.scene = std::move(ps.scene), json.maxDepth = ps.maxDepth, json.samplesPerPixel = ps.samplesPerPixel;
    } else {
      ok = dmt_host::loadJsonScene(cfg.scenePath, json, &err);
    }
    if (!ok) {
      std::fprintf(stderr, "scene '%s': %s\n", cfg.scenePath.c_str(), err.c_str());
      return 1;
    }
    if (!cfg.widthSet) cfg.width = json.scene.camera.width;
    if (!cfg.heightSet) cfg.height = json.scene.camera.height;
    if (!cfg.sppSet) cfg.spp = json.samplesPerPixel;
    if (!cfg.depthSet) cfg.maxDepth = json.maxDepth;
    if (cfg.kspp > cfg.spp) cfg.kspp = cfg.spp;
  }
  dmt_host::Scene key1;  // --motion-scene: only its triangle positions are used
  if (!cfg.motionScenePath.empty()) {
    std::string err;
    std::string const& path = cfg.motionScenePath;
    bool ok;
    if (path.size() > 5 && path.compare(path.size() - 5, 5, ".pbrt") == 0) {
      dmt_host::PbrtScene ps;
      ok = dmt_host::loadPbrtScene(path, ps, &err);
      key1 = std::move(ps.scene);
    } else {
      dmt_host::JsonScene js;
      ok = dmt_host::loadJsonScene(path, js, &err);
      key1 = std::move(js.scene);
    }
    if (!ok) {
      std::fprintf(stderr, "motion scene '%s': %s\n", path.c_str(), err.c_str());
      return 1;
    }
    size_t const want = cfg.scenePath.empty() ? dmt_host::cornellBox().triangleCount() : json.scene.triangleCount();
    if (key1.triangleCount() != want) {
      std::fprintf(stderr, "motion scene '%s': %zu triangles, the scene has %zu: key 1 must move the same triangles\n", path.c_str(),
                   key1.triangleCount(), want);
      return 1;
    }
  }
  if (std::string const err = cfg.validate(); !err.empty()) {
    std::fprintf(stderr, "%s\n", err.c_str());
    printHelp();
    return 1;
  }
  if (cfg.adaptive) Config::parseThreshold(cfg.adaptiveArg, cfg.threshold);
  Config::parseShadingNormals(cfg.shadingNormals, cfg.creaseDegrees);
  std::printf("Parsed Configuration:\n - Width:     %d\n - Height:    %d\n - SPP:       %d\n - KSPP:      %d\n - Log Level: %s\n",
              cfg.width, cfg.height, cfg.spp, cfg.kspp, cfg.logLevel.c_str());
  bool const verbose = cfg.logLevel == "verbose";
  dmt_host::Scene scene = cfg.scenePath.empty() ? dmt_host::cornellBox() : std::move(json.scene);
  scene.camera.width = cfg.width, scene.camera.height = cfg.height, scene.camera.spp = cfg.kspp;
  if (cfg.textureFilter) scene.camera.spp = cfg.spp;  // the filter's footprint scale follows the frame's samples per pixel
  if (cfg.lensRadiusSet) scene.lensRadius = cfg.lensRadius;
  if (cfg.focusDistanceSet) scene.focusDistance = cfg.focusDistance;
  if (!cfg.projection.empty()) {  // --projection replaces the scene file's
    scene.projection = cfg.projection == "orthographic" ? DMT_PROJECTION_ORTHOGRAPHIC : cfg.projection == "equirect" ? DMT_PROJECTION_EQUIRECT
                       : cfg.projection == "fisheye"    ? DMT_PROJECTION_FISHEYE : DMT_PROJECTION_PERSPECTIVE;
    scene.projectionParam = cfg.orthoHeightSet ? cfg.orthoHeight : cfg.fisheyeFovSet ? cfg.fisheyeFov : 0.f;
  }
  if (scene.projection != DMT_PROJECTION_PERSPECTIVE) {  // what the library refuses under the projection, before anything is rendered
    char const* why = nullptr;
    if (scene.lensRadius > 0.f) why = "dmt_set_projection: a thin lens (dmt_set_lens, radius > 0) is set; only the perspective camera has one";
    else if (cfg.denoise) why = "dmt_denoise: the depth scale and the reprojection are the perspective camera's (dmt_set_projection set another projection)";
    else if (cfg.textureFilter) why = "dmt_render: the first-hit texture filter together with another projection than the perspective one (dmt_set_projection) is not supported";
    else if (cfg.focusPixelSet) why = "dmt_focus_distance_at: the autofocus ray is the pinhole's (dmt_set_projection set another projection)";
    if (why) {
      std::fprintf(stderr, "--projection / the scene's projection: %s\n", why);
      return 1;
    }
  }
  if (cfg.mediumSet) {  // --medium replaces the scene file's medium; the default box is the bounds of the triangles
    scene.hasMedium = cfg.mediumSigmaT > 0.f, scene.mediumSigmaT = cfg.mediumSigmaT, scene.mediumG = cfg.mediumG;
    for (int i = 0; i < 3; ++i) scene.mediumAlbedo[i] = cfg.mediumAlbedo[i];
    for (int i = 0; i < 3; ++i) scene.mediumExtinction[i] = cfg.mediumExtinction[i], scene.mediumEmission[i] = cfg.mediumEmission[i];
    for (int i = 0; i < 3 && cfg.mediumBoxSet; ++i) scene.mediumMin[i] = cfg.mediumBox[i], scene.mediumMax[i] = cfg.mediumBox[3 + i];
    if (!cfg.mediumBoxSet) {
      std::vector<float> const* const axes[3] = {&scene.xs, &scene.ys, &scene.zs};
      for (int a = 0; a < 3; ++a) {
        float lo = std::numeric_limits<float>::infinity(), hi = -lo;
        for (size_t t = 0; t < scene.triangleCount(); ++t)
          for (size_t c = 0; c < 3; ++c) lo = std::min(lo, (*axes[a])[4 * t + c]), hi = std::max(hi, (*axes[a])[4 * t + c]);
        scene.mediumMin[a] = lo, scene.mediumMax[a] = hi;
        if (scene.hasMedium && !(lo < hi)) {
          std::fprintf(stderr, "--medium: the scene's triangles span no volume; give --medium-box\n");
          return 1;
        }
      }
    }
  }
  if (!cfg.mediumGridPath.empty()) {  // --medium-grid replaces the scene file's grid; checked before any GPU is touched
    if (!scene.hasMedium) {
      std::fprintf(stderr, "--medium-grid needs a medium, from --medium or the scene file\n");
      return 1;
    }
    std::string err;
    if (!dmt_host::readNpyGrid(cfg.mediumGridPath, scene.mediumGrid, scene.mediumGridDims, &err)) {
      std::fprintf(stderr, "--medium-grid: %s\n", err.c_str());
      return 1;
    }
  }
  if (scene.hasMedium && scene.mediumSigmaT > 0.f && cfg.denoise) {
    std::fprintf(stderr, "the scene's medium and --denoise exclude each other (the feature buffers do not know the fog)\n");
    return 1;
  }
  // --pixel-filter: the scene file's filter applies only with "scene"; a kind given here replaces it; without the option none is set
  if (cfg.pixelFilter.empty()) {
    scene.pixelFilterKind = dmt_host::Scene::kNoPixelFilter;
  } else if (cfg.pixelFilter == "scene") {
    if (scene.pixelFilterKind == dmt_host::Scene::kNoPixelFilter) {
      std::fprintf(stderr, "--pixel-filter scene: the scene records no pixel filter\n");
      return 1;
    }
    if (scene.pixelFilterKind == dmt_host::Scene::kUnsupportedPixelFilter) {
      std::fprintf(stderr, "--pixel-filter scene: the scene's pixel filter '%s' is an unsupported kind\n", scene.pixelFilterName.c_str());
      return 1;
    }
  } else {
    dmt_host::recordPixelFilter(scene, cfg.pixelFilter, cfg.filterRadiusSet ? cfg.filterRadius : -1.f, cfg.filterSigmaSet ? cfg.filterSigma : -1.f);
  }
  if (cfg.cutouts == "off") scene.matOpacity.clear();  // --cutouts off: uploadScene then uploads no opacity
  std::vector<float> vertexNormals;  // --shading-normals: 9 floats per triangle for dmt_upload_vertex_normals
  if (cfg.shadingNormals == "file") {
    if (scene.triNormals.size() != 9 * scene.triangleCount()) {
      std::fprintf(stderr, "--shading-normals file: the scene's meshes carry no vertex normals (try --shading-normals smooth)\n");
      return 1;
    }
    vertexNormals = scene.triNormals;
  } else if (cfg.shadingNormals != "off") {
    vertexNormals.resize(9 * scene.triangleCount());
    if (dmt_smooth_normals(scene.xs.data(), scene.ys.data(), scene.zs.data(), scene.triangleCount(), cfg.creaseDegrees, vertexNormals.data()) != DMT_OK) {
      std::fprintf(stderr, "--shading-normals smooth: dmt_smooth_normals failed\n");
      return 1;
    }
  }
  double const loadMs = msSince(tLoad);

  // one context per GPU; DMT_CLI_SHARE_DEVICE=1 (tests on a one-GPU box) maps all ranks onto --gpu-ordinal
  auto const tUpload = std::chrono::steady_clock::now();
  bool const share = std::getenv("DMT_CLI_SHARE_DEVICE") != nullptr;
  Contexts C;
  C.v.assign(size_t(cfg.gpus), nullptr);
  for (int r = 0; r < cfg.gpus; ++r) {
    if (dmt_ctx_create(share ? cfg.device : cfg.device + r, &C.v[size_t(r)]) != DMT_OK) return fail(nullptr, "dmt_ctx_create");
    dmt_ctx* ctx = C.v[size_t(r)];
    if (dmt_host::uploadScene(ctx, scene) != DMT_OK) return fail(ctx, "uploadScene");
    if (std::string err; dmt_host::applyPixelFilter(ctx, scene, err) != DMT_OK) {  // every rank sets it on its own context, as the lens
      std::fprintf(stderr, "pixel filter: %s\n", err.c_str());
      return 1;
    }
    if (dmt_set_limits(ctx, cfg.maxDepth) != DMT_OK) return fail(ctx, "dmt_set_limits");
    if (cfg.bvhBuildSet && dmt_set_accel_build(ctx, cfg.bvhBuildArg == "gpu" ? DMT_BVH_BUILD_DEVICE : DMT_BVH_BUILD_HOST) != DMT_OK)
      return fail(ctx, "dmt_set_accel_build");
    if (cfg.bvh && dmt_set_accel(ctx, DMT_ACCEL_BVH) != DMT_OK) return fail(ctx, "dmt_set_accel");
    if (dmt_set_partition(ctx, r, cfg.gpus) != DMT_OK) return fail(ctx, "dmt_set_partition");
    if (cfg.lightTree && dmt_set_light_sampling(ctx, DMT_LIGHTS_TREE) != DMT_OK) return fail(ctx, "dmt_set_light_sampling");
    if (cfg.emitterTree && dmt_set_emitter_sampling(ctx, DMT_EMITTERS_TREE) != DMT_OK) return fail(ctx, "dmt_set_emitter_sampling");
    if (cfg.lightTreeRef && dmt_set_light_sampling(ctx, DMT_LIGHTS_TREE_REFERENCE) != DMT_OK) return fail(ctx, "dmt_set_light_sampling");
    if (cfg.textureFilter && dmt_set_texture_filter(ctx, DMT_TEXFILTER_REFERENCE) != DMT_OK) return fail(ctx, "dmt_set_texture_filter");
    if (cfg.shutterSet && dmt_set_shutter(ctx, cfg.shutterOpen, cfg.shutterClose) != DMT_OK) return fail(ctx, "dmt_set_shutter");
    if (!cfg.motionScenePath.empty() && dmt_set_motion(ctx, key1.xs.data(), key1.ys.data(), key1.zs.data(), key1.triangleCount()) != DMT_OK)
      return fail(ctx, "dmt_set_motion");
    if (!vertexNormals.empty() && dmt_upload_vertex_normals(ctx, vertexNormals.data(), scene.triangleCount()) != DMT_OK)
      return fail(ctx, "dmt_upload_vertex_normals");
  }
  if (cfg.focusPixelSet) {  // autofocus on the first context (every context holds the whole scene), then the lens of all
    float d = 0.f;
    if (dmt_focus_distance_at(C.v[0], std::floor(cfg.focusX) + 0.5f, std::floor(cfg.focusY) + 0.5f, &d) != DMT_OK)
      return fail(C.v[0], "dmt_focus_distance_at");
    std::printf("Autofocus: pixel (%d, %d) -> focus distance %.6g\n", int(cfg.focusX), int(cfg.focusY), double(d));
    for (dmt_ctx* ctx : C.v)
      if (dmt_set_lens(ctx, scene.lensRadius, d) != DMT_OK) return fail(ctx, "dmt_set_lens");
  }
  double const uploadMs = msSince(tUpload);

  std::string const dir = cfg.outDir.empty() ? executableDirectory() : cfg.outDir;
  size_t const pixels = size_t(cfg.width) * size_t(cfg.height);
  std::vector<float> mean(4 * pixels), m2(4 * pixels), pm, pm2;
  double downloadMs = 0.0, writeMs = 0.0;
  int lastSamples = 0;  // the <spp> of the last output-<spp>.png
  auto writeOut = [&](int samples) {
    lastSamples = samples;
    auto const t0 = std::chrono::steady_clock::now();
    if (dmt_download_film(C.v[0], mean.data(), m2.data()) != DMT_OK) return fail(C.v[0], "dmt_download_film"), false;
    if (cfg.gpus > 1) {  // disjoint tile sets over zero-initialised frames: the sum is an exact gather
      pm.resize(4 * pixels), pm2.resize(4 * pixels);
      for (int r = 1; r < cfg.gpus; ++r) {
        if (dmt_download_film(C.v[size_t(r)], pm.data(), pm2.data()) != DMT_OK) return fail(C.v[size_t(r)], "dmt_download_film"), false;
        for (size_t i = 0; i < 4 * pixels; ++i) mean[i] += pm[i], m2[i] += pm2[i];
      }
    }
    downloadMs += msSince(t0);
    auto const t1 = std::chrono::steady_clock::now();
    std::string err;
    std::puts("Writing to file");
    if (!dmt_host::writeMeanAndMSERowMajor(mean.data(), m2.data(), uint32_t(cfg.width), uint32_t(cfg.height),
                                           dir + "/output-" + std::to_string(samples), &err)) {
      std::fprintf(stderr, "%s\n", err.c_str());
      return false;
    }
    writeMs += msSince(t1);
    return true;
  };

  std::puts("Running HIP Kernel");
  double totalMs = 0.0;  // wall time of launch + sync, file writes excluded (main.cu:179-192)
  int launches = 0;
  uint64_t adaptiveSamples = 0;  // --adaptive: path samples traced over all GPUs
  if (cfg.adaptive) {  // synchronous per context (one read-back per round), so the GPUs run their shares one after another
    auto const t0 = std::chrono::steady_clock::now();
    for (dmt_ctx* ctx : C.v) {
      uint32_t rounds = 0;
      uint64_t traced = 0;
      if (dmt_render_adaptive(ctx, uint32_t(cfg.minSpp), uint32_t(cfg.spp), uint32_t(cfg.kspp), cfg.threshold, 0, 0, cfg.width,
                              cfg.height, &rounds, &traced) != DMT_OK)
        return fail(ctx, "dmt_render_adaptive");
      if (dmt_sync(ctx) != DMT_OK) return fail(ctx, "dmt_sync");
      launches = std::max(launches, int(rounds)), adaptiveSamples += traced;
    }
    totalMs += msSince(t0);
  }
  for (int sTot = 0; !cfg.adaptive && sTot < cfg.spp; sTot += cfg.kspp) {
    if (verbose) std::printf("Running HIP Kernel (%d)\n", sTot);
    auto const t0 = std::chrono::steady_clock::now();
    for (dmt_ctx* ctx : C.v)  // asynchronous: all GPUs run their share of this batch concurrently
      if (dmt_render(ctx, uint32_t(sTot), uint32_t(cfg.kspp), 0, 0, cfg.width, cfg.height) != DMT_OK) return fail(ctx, "dmt_render");
    for (dmt_ctx* ctx : C.v)
      if (dmt_sync(ctx) != DMT_OK) return fail(ctx, "dmt_sync");
    totalMs += msSince(t0);
    ++launches;
    if (cfg.savePartial && !writeOut(sTot + cfg.kspp)) return 1;
  }
  if (!cfg.savePartial && !writeOut(cfg.spp)) return 1;
  if (cfg.adaptive) {  // grey map of the samples each pixel received, N / spp
    auto const t1 = std::chrono::steady_clock::now();
    std::vector<uint8_t> grey(3 * pixels);
    for (size_t i = 0; i < pixels; ++i)
      grey[3 * i] = grey[3 * i + 1] = grey[3 * i + 2] = uint8_t(std::lround(255.0 * std::min(1.0, double(m2[4 * i + 3]) / double(cfg.spp))));
    std::string err;
    if (!dmt_host::writePngRgb8(dir + "/output-" + std::to_string(cfg.spp) + "_spp.png", grey.data(), uint32_t(cfg.width),
                                uint32_t(cfg.height), &err)) {
      std::fprintf(stderr, "%s\n", err.c_str());
      return 1;
    }
    writeMs += msSince(t1);
  }
  double aovMs = 0.0, denoiseMs = 0.0;
  float denoiseKernelMs = 0.f;
  std::vector<float> den;  // --denoise: the filtered plane, kept for the display transform
  if (cfg.denoise) {  // feature buffers on the first context (they cover the whole frame), filter on the combined host film
    auto const t0 = std::chrono::steady_clock::now();
    if (dmt_render_aovs(C.v[0], uint32_t(cfg.aovSpp)) != DMT_OK) return fail(C.v[0], "dmt_render_aovs");
    if (dmt_sync(C.v[0]) != DMT_OK) return fail(C.v[0], "dmt_sync");
    aovMs = msSince(t0);
    auto const t1 = std::chrono::steady_clock::now();
    den.resize(4 * pixels);
    if (dmt_denoise(C.v[0], nullptr, mean.data(), m2.data(), den.data(), &denoiseKernelMs) != DMT_OK) return fail(C.v[0], "dmt_denoise");
    denoiseMs = msSince(t1);
    auto const t2 = std::chrono::steady_clock::now();
    std::vector<uint8_t> rgb(3 * pixels);
    dmt_host::filmToRgb8(den.data(), m2.data(), pixels, rgb.data(), nullptr);  // the quantisation of output-<spp>.png
    std::string err;
    if (!dmt_host::writePngRgb8(dir + "/output-" + std::to_string(lastSamples) + "_denoised.png", rgb.data(), uint32_t(cfg.width),
                                uint32_t(cfg.height), &err)) {
      std::fprintf(stderr, "%s\n", err.c_str());
      return 1;
    }
    writeMs += msSince(t2);
  }
  double displayMs = 0.0;
  float displayKernelMs = 0.f;
  dmt_display_record displayRec{};
  if (cfg.display) {  // on the first context, from the combined host film, as the denoiser
    dmt_display_params const dp = cfg.displayParams();
    std::vector<uint8_t> rgba(4 * pixels), rgb(3 * pixels);
    auto show = [&](float const* plane, std::string const& name) {
      auto const t0 = std::chrono::steady_clock::now();
      float ms = 0.f;
      if (dmt_display(C.v[0], &dp, plane, nullptr, rgba.data(), &ms) != DMT_OK) return fail(C.v[0], "dmt_display"), false;
      displayMs += msSince(t0), displayKernelMs += ms;
      auto const t1 = std::chrono::steady_clock::now();
      for (size_t i = 0; i < pixels; ++i) rgb[3 * i] = rgba[4 * i], rgb[3 * i + 1] = rgba[4 * i + 1], rgb[3 * i + 2] = rgba[4 * i + 2];
      std::string err;
      if (!dmt_host::writePngRgb8(dir + "/output-" + std::to_string(lastSamples) + name, rgb.data(), uint32_t(cfg.width), uint32_t(cfg.height), &err)) {
        std::fprintf(stderr, "%s\n", err.c_str());
        return false;
      }
      writeMs += msSince(t1);
      return true;
    };
    if (!show(mean.data(), "_display.png")) return 1;
    if (dmt_display_info(C.v[0], &displayRec) != DMT_OK) return fail(C.v[0], "dmt_display_info");  // the film's, not the denoised plane's
    if (cfg.denoise && !show(den.data(), "_denoised_display.png")) return 1;
  }
  if (cfg.hdr) {
    auto const t0 = std::chrono::steady_clock::now();
    std::string err;
    if (!dmt_host::writePfmRgb(dir + "/output-" + std::to_string(lastSamples) + ".pfm", mean.data(), uint32_t(cfg.width), uint32_t(cfg.height), &err)) {
      std::fprintf(stderr, "%s\n", err.c_str());
      return 1;
    }
    writeMs += msSince(t0);
  }
  double const samples = cfg.adaptive ? double(adaptiveSamples) : double(pixels) * double(launches) * double(cfg.kspp);
  std::printf("Done! Total Execution Time(excl write file): %llu ms | Average Execution per Kernel launch (%d spp): %llu ms | %.2f Msamples/s\n",
              static_cast<unsigned long long>(totalMs), cfg.kspp, static_cast<unsigned long long>(totalMs / std::max(launches, 1)),
              samples / (totalMs * 1e3));
  if (cfg.timeReport) {  // --time: execution times of the key operations (cli/CLIManager.cpp:27-31)
    double kernelMs = 0.0;
    uint64_t n = 0;
    for (dmt_ctx* ctx : C.v) {
      double ms = 0.0;
      uint64_t k = 0;
      if (dmt_kernel_time(ctx, &ms, &k, 1) == DMT_OK && ms > kernelMs) kernelMs = ms, n = k;
    }
    std::printf("Timing report:\n - scene load / build:        %10.3f ms\n - context + upload%s: %10.3f ms (%d GPU%s)\n"
                " - render (launch + sync):    %10.3f ms in %d launch(es) of %d spp\n"
                " - kernels (HIP events, max over GPUs): %10.3f ms in %llu launch(es)\n"
                " - film download%s:   %10.3f ms\n - PNG encode + write:       %10.3f ms\n",
                loadMs, cfg.bvh ? " + BVH build" : "            ", uploadMs, cfg.gpus, cfg.gpus > 1 ? "s" : "", totalMs, launches, cfg.kspp,
                kernelMs, static_cast<unsigned long long>(n), cfg.gpus > 1 ? " + gather" : "         ", downloadMs, writeMs);
    if (cfg.bvhBuildSet) {  // the build record of the first context's tree
      dmt_accel_build_record rec{};
      if (dmt_accel_build_info(C.v[0], &rec) != DMT_OK) return fail(C.v[0], "dmt_accel_build_info");
      char const* const who = rec.builder == DMT_BVH_BUILT_BY_DEVICE ? "gpu" : rec.builder == DMT_BVH_BUILT_BY_HOST ? "host" : "host, after the gpu build was abandoned as too deep";
      std::printf(" - BVH build:                 %10.3f ms (%s): %u triangles -> %u nodes, %u pairs, depth %d, %.1f MB of device temporaries\n",
                  rec.build_ms, who, rec.triangles, rec.nodes, rec.pairs, int(rec.depth), double(rec.temp_bytes) / 1e6);
    }
    if (cfg.adaptive)
      std::printf(" - adaptive sampling:         %d round(s), %llu samples traced (%.2f spp on average, cap %d)\n", launches,
                  static_cast<unsigned long long>(adaptiveSamples), double(adaptiveSamples) / double(pixels), cfg.spp);
    if (cfg.denoise)
      std::printf(" - denoise:                   AOVs %.3f ms (%d spp, launch + sync), filter %.3f ms (kernels, HIP events; %.3f ms with copies)\n",
                  aovMs, cfg.aovSpp, double(denoiseKernelMs), denoiseMs);
    if (cfg.display)
      std::printf(" - display:                   %.3f ms (kernels, HIP events; %.3f ms with copies), exposure scale %.6g%s, %d bloom level(s)\n",
                  double(displayKernelMs), displayMs, double(displayRec.scale), cfg.exposure == "auto" ? " (metered)" : "", int(displayRec.levels));
  }
  std::puts("Cleanup...");
  return 0;
}
