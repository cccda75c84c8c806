"""MI355X-native path-tracing hot path (drop-in for the reference's megakernel launch boundary).

The product is the C-ABI shared library ``csrc/libdmt_hip.so`` (see ``include/dmt_hip.h``) plus the
C++ host side in ``host/``.  This Python package is only the ctypes plumbing that tests and
``bench.py`` use to call through that C ABI; it contains no rendering logic and NO fallback:
if the HIP library is missing or no GPU is present, calls raise.

The directory name contains a hyphen, so import it through ``__graft_entry__.load_package()`` (or
``tests/conftest.py``), which registers it as ``cuda_optix_pathtracing_amd``.
"""
from .binding import (  # noqa: F401
    DmtError,
    Renderer,
    bvh_validate,
    bvh_check,
    lbvh_reference,
    BVH_BUILD_HOST,
    BVH_BUILD_DEVICE,
    BVH_BUILT_BY_HOST,
    BVH_BUILT_BY_DEVICE,
    BVH_BUILT_BY_HOST_AFTER_DEVICE,
    bvh_refit_reference,
    BVH_UPDATE_REBUILD,
    BVH_UPDATE_REFIT,
    BVH_UPDATE_AUTO,
    BVH_UPDATED_NONE,
    BVH_UPDATED_REFIT,
    BVH_UPDATED_REBUILD,
    BVH_UPDATED_REBUILD_AFTER_REFIT,
    light_tree_pmfs,
    light_tree_ref_select,
    light_tree_nodes,
    LIGHT_TREE_NODE,
    LIGHT_TREE_REF_NODE,
    LIGHT_TREE_LEAF,
    emitter_tree_nodes,
    emitter_tree_select,
    emitter_tree_pmfs,
    EMITTER_TREE_NODE,
    EMITTER_TREE_LEAF,
    EMITTERS_UNIFORM,
    EMITTERS_TREE,
    envmap_tables,
    texture_mip_chain,
    texture_footprint,
    temporal_defaults,
    camera_project,
    lens_rays,
    shutter_times,
    motion_positions,
    motion_bvh_validate,
    smooth_normals,
    opacity_eval,
    OPACITY_NONE,
    medium_segment,
    medium_values,
    phase_hg,
    medium_grid_march,
    medium_spectrum_event,
    mip_level_count,
    TEXFILTER_LEVEL0,
    TEXFILTER_REFERENCE,
    build_library,
    library_path,
    load_library,
)
from . import host_scene  # noqa: F401,E402
from . import multigpu  # noqa: F401,E402
