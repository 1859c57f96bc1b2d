"""ctypes binding of include/immesh_c_api.h.

``HotPath(lib, prefix)`` wraps one context.  The same wrapper drives the product (``prefix='immesh_'``,
libimmesh_hip.so) and -- from tests/bench only -- the CPU oracle (``prefix='orc_'``, oracle/liboracle.so), which
exports the identical entry points.  Nothing here computes anything.
"""
import ctypes as C
import os
import sys
import numpy as np

STATE_DOUBLES = 348
_HERE = os.path.dirname(os.path.abspath(__file__))


RUNTIME_CHOICE = None


def one_hip_runtime():
    """ONE HIP / HSA runtime in a test or bench process.

    The torch wheel bundles its own copies of libamdhip64 / libhsa-runtime64 and its libraries ask for them by the bare file names
    ``libamdhip64.so`` / ``libhsa-runtime64.so``; the product library is linked against the system copies (/opt/rocm) by soname.  The loader reuses
    an object that is already mapped under the name asked for, so WHO IS MAPPED FIRST decides, and this function fixes it:

    * single-GPU processes (the GPU test tier, smoke, ``bench.py --gpus 1``): the SYSTEM copies are mapped under exactly the names torch asks for
      BEFORE torch is imported, so torch runs on them too -- one runtime, and it is the one the reference's process would have (there is no torch
      there), with torch as the guest (measured on an MI355X box: device ops, a GEMM, a world-1 RCCL all-reduce -- tools/r05_one_runtime.py);
    * ranks of a multi-GPU job (WORLD_SIZE > 1): torch -- whose bundle of runtime + RCCL is the combination that is exercised together everywhere
      -- is imported first, and the library binds to ITS copy by soname: still one runtime, no mix of an RCCL built for one runtime on another
      where it cannot be tried beforehand (this container has no multi-GPU box);
    * torch already imported by the caller: its copy is the process's runtime; nothing to do.

    IMMESH_RUNTIME = system | torch | none overrides the choice: ``none`` leaves the loader alone -- for an application that embeds this
    binding next to its own torch and does not want the system ROCm mapped under torch's file names; ``torch`` / ``system`` force one of the two
    arrangements above.  This is loader policy of the TEST / BENCH binding only: the product (libimmesh_hip.so behind include/immesh_c_api.h, loaded by a
    C++ node) does none of it.

    Returns the runtime files mapped."""
    global RUNTIME_CHOICE
    forced = os.environ.get("IMMESH_RUNTIME", "").strip().lower()
    if forced == "none":
        RUNTIME_CHOICE = "untouched (IMMESH_RUNTIME=none)"
        return mapped_hip_runtimes()
    if forced == "torch" and "torch" not in sys.modules:
        RUNTIME_CHOICE = "torch (IMMESH_RUNTIME=torch)"
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        return mapped_hip_runtimes()
    if "torch" in sys.modules:
        RUNTIME_CHOICE = "torch (imported before the binding)"
    else:
        if int(os.environ.get("WORLD_SIZE", "1") or 1) > 1 and os.environ.get("IMMESH_SYSTEM_RUNTIME", "") != "1" and forced != "system":
            RUNTIME_CHOICE = "torch (rank of a multi-GPU job)"
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        else:
            RUNTIME_CHOICE = "system"
            for name in ("libhsa-runtime64.so", "libamdhip64.so"):
                try:
                    C.CDLL(name, mode=C.RTLD_GLOBAL)
                except OSError:
                    pass                  # no ROCm in the loader's cache (a CPU-only box): the library load below fails loudly on its own
    return mapped_hip_runtimes()


def mapped_hip_runtimes():
    out = set()
    try:
        with open("/proc/self/maps") as f:
            for ln in f:
                if "libamdhip64" in ln or "libhsa-runtime64" in ln:
                    out.add(ln.split()[-1])
    except OSError:
        pass
    return sorted(out)


one_hip_runtime()


class Config(C.Structure):
    _fields_ = [
        ("voxel_size", C.c_double), ("max_layer", C.c_int32), ("layer_init", C.c_int32 * 5), ("max_points_size", C.c_int32),
        ("planer_threshold", C.c_double), ("dept_err", C.c_double), ("beam_err", C.c_double), ("calib_laser", C.c_int32),
        ("sigma_num", C.c_double), ("max_iter", C.c_int32), ("extR", C.c_double * 9), ("extT", C.c_double * 3),
        ("mesh_min_spacing", C.c_double), ("mesh_voxel", C.c_double), ("mesh_region", C.c_double), ("mesh_append_budget", C.c_int32),
        ("device", C.c_int32), ("cap_root_voxels", C.c_int64), ("cap_nodes", C.c_int64), ("cap_point_chunks", C.c_int64),
        ("cap_vertices", C.c_int64), ("cap_triangles", C.c_int64), ("cap_scan_points", C.c_int64),
        ("shard_rank", C.c_int32), ("shard_world", C.c_int32), ("shard_brick_log2", C.c_int32), ("shard_mesh", C.c_int32),
        ("shard_scheme", C.c_int32), ("reserved_", C.c_int32),
    ]


class MeshSizes(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("vtx_base", "n_new_vtx", "n_add", "n_rem", "n_upd", "n_smooth", "n_voxels_meshed", "reserved")]


class PlaneRec(C.Structure):
    _fields_ = [("key", C.c_int64 * 3), ("layer", C.c_int32), ("path", C.c_int32), ("is_plane", C.c_int32), ("n_points", C.c_int32),
                ("update_enable", C.c_int32), ("new_points", C.c_int32), ("radius", C.c_float), ("min_eig", C.c_float), ("d", C.c_float),
                ("pad", C.c_float), ("center", C.c_double * 3), ("normal", C.c_double * 3), ("plane_var", C.c_double * 36)]


PLANE_DTYPE = np.dtype([("key", "<i8", 3), ("layer", "<i4"), ("path", "<i4"), ("is_plane", "<i4"), ("n_points", "<i4"),
                        ("update_enable", "<i4"), ("new_points", "<i4"), ("radius", "<f4"), ("min_eig", "<f4"), ("d", "<f4"),
                        ("pad", "<f4"), ("center", "<f8", 3), ("normal", "<f8", 3), ("plane_var", "<f8", 36)])
assert PLANE_DTYPE.itemsize == C.sizeof(PlaneRec)

COUNTER_FIELDS = ("n_ds", "n_iter", "n_match", "n_plane_tests", "n_extra_probe", "n_refits", "n_refit_pts", "n_app", "n_new", "v_act",
                  "n_v", "n_u", "t_v", "t_add", "t_rem", "c1", "c20", "n_root_voxels", "n_nodes", "n_vertices", "n_triangles_live", "n_degenerate_skips")


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 56), ("launches", C.c_int64), ("total_ms", C.c_double)]


class Camera(C.Structure):
    """immesh_camera (include/immesh_render.h): the depth view of LiDAR point reinforcement"""
    _fields_ = [("rot", C.c_double * 9), ("pos", C.c_double * 3), ("width", C.c_int32), ("height", C.c_int32), ("focus", C.c_double),
                ("z_near", C.c_double), ("z_far", C.c_double), ("downsample_res", C.c_double)]


def default_depth_camera(lib, **over):
    """immesh_default_depth_camera (640 x 480, focus 400, 0.05 / 200, cell 0.01, identity pose) with fields overridden by keyword"""
    cam = Camera()
    lib.immesh_default_depth_camera.argtypes = [C.POINTER(Camera)]; lib.immesh_default_depth_camera.restype = None
    lib.immesh_default_depth_camera(C.byref(cam))
    for k, v in over.items():
        if k in ("rot", "pos"):
            getattr(cam, k)[:] = [float(x) for x in np.asarray(v, float).reshape(-1)]
        else:
            setattr(cam, k, v)
    return cam


def camera_from_state(lib, state, cam=None):
    """immesh_camera_from_state: the pose of `cam` (default: the default depth camera) from a state vector (make_state layout)"""
    cam = default_depth_camera(lib) if cam is None else cam
    st = np.ascontiguousarray(state, dtype=np.float64)
    f = lib.immesh_camera_from_state; f.argtypes = [C.c_void_p, C.POINTER(Camera)]; f.restype = C.c_int
    rc = f(st.ctypes.data_as(C.c_void_p), C.byref(cam))
    if rc != 0:
        raise RuntimeError(f"immesh_camera_from_state failed rc={rc}")
    return cam


class RayFrame(C.Structure):
    """immesh_ray_frame (include/immesh_raycast.h): sensor-to-world rotation (row-major) and the sensor origin in the world"""
    _fields_ = [("rot", C.c_double * 9), ("pos", C.c_double * 3)]


assert C.sizeof(RayFrame) == 96
RAY_NEAREST, RAY_ANY = 0, 1


def ray_frame(rot=None, pos=None):
    """a RayFrame from a 3 x 3 rotation and a position (identity / origin by default)"""
    fr = RayFrame()
    fr.rot[:] = [float(x) for x in (np.eye(3) if rot is None else np.asarray(rot, float)).reshape(-1)]
    fr.pos[:] = [float(x) for x in (np.zeros(3) if pos is None else np.asarray(pos, float)).reshape(-1)]
    return fr


class ClosestStats(C.Structure):
    """immesh_closest_stats (include/immesh_closest.h): the last closest-point query reduced on the device"""
    _fields_ = [("n_points", C.c_int64), ("n_with_face", C.c_int64), ("n_not_finite", C.c_int64), ("n_no_face", C.c_int64), ("n_overflow", C.c_int64),
                ("sum_dist", C.c_double), ("sum_dist2", C.c_double), ("mean", C.c_double), ("rms", C.c_double),
                ("max_dist", C.c_float), ("bin_width", C.c_float)]


class AlignOptions(C.Structure):
    """immesh_align_options (include/immesh_align.h)"""
    _fields_ = [("mode", C.c_int32), ("max_iters", C.c_int32), ("max_dist", C.c_double), ("centre", C.c_double * 3), ("damping", C.c_double),
                ("eps_rot", C.c_double), ("eps_trans", C.c_double)]


class AlignSystem(C.Structure):
    """immesh_align_system (include/immesh_align.h): the 28 sums of a step (H a <= b row by row, g, e) and its four counts"""
    _fields_ = [("H", C.c_double * 21), ("g", C.c_double * 6), ("e", C.c_double),
                ("n_used", C.c_int64), ("n_not_finite", C.c_int64), ("n_no_face", C.c_int64), ("n_flat", C.c_int64)]

    def sums(self):
        """the 28 sums in the terms' order -> (28,) float64"""
        return np.array(list(self.H) + list(self.g) + [self.e], np.float64)

    def counts(self):
        return self.n_used, self.n_not_finite, self.n_no_face, self.n_flat


class AlignResult(C.Structure):
    """immesh_align_result (include/immesh_align.h)"""
    _fields_ = [("frame", RayFrame), ("status", C.c_int32), ("iterations", C.c_int32), ("system", AlignSystem), ("rms", C.c_double)]


assert (C.sizeof(AlignOptions), C.sizeof(AlignSystem), C.sizeof(AlignResult)) == (64, 256, 368)
ALIGN_POINT, ALIGN_PLANE = 0, 1
ALIGN_CONVERGED, ALIGN_MAX_ITERS, ALIGN_TOO_FEW, ALIGN_DEGENERATE = 0, 1, 2, 3
ALIGN_STATUS = ("converged", "max_iters", "too_few", "degenerate")
ALIGN_TERMS = 28


def align_options(mode=ALIGN_POINT, max_dist=1.0, centre=(0.0, 0.0, 0.0), damping=0.0, max_iters=30, eps_rot=1e-9, eps_trans=1e-9):
    """an AlignOptions (the defaults are immesh_align_default_options'); centre: three numbers (align() also takes "mean")"""
    o = AlignOptions(mode=mode, max_iters=max_iters, max_dist=max_dist, damping=damping, eps_rot=eps_rot, eps_trans=eps_trans)
    o.centre[:] = [float(x) for x in centre]
    return o


def align_centre_mean(pts, frame=None):
    """the mean of the finite points under `frame` (None: as they are), in float64 -> [x, y, z]; zeros without a finite point"""
    p = np.asarray(pts, np.float32).reshape(-1, 3)
    p = p[np.isfinite(p).all(axis=1)].astype(np.float64)
    if len(p) == 0:
        return [0.0, 0.0, 0.0]
    m = p.mean(axis=0)
    if frame is not None:
        m = np.array(list(frame.rot)).reshape(3, 3) @ m + np.array(list(frame.pos))
    return [float(x) for x in m]


def align_solve(lib, system, damping=0.0):
    """immesh_align_solve (pure host code, no context) -> (degenerate, delta (6,) float64)"""
    f = lib.immesh_align_solve; f.argtypes = [C.POINTER(AlignSystem), C.c_double, C.c_void_p]; f.restype = C.c_int
    delta = np.zeros(6, np.float64)
    rc = f(C.byref(system), damping, _ptr(delta))
    if rc not in (0, 1):
        raise RuntimeError(f"immesh_align_solve failed rc={rc}")
    return rc == 1, delta


def align_update(lib, frame, centre, delta):
    """immesh_align_update (pure host code, no context) -> RayFrame"""
    f = lib.immesh_align_update; f.argtypes = [C.POINTER(RayFrame), C.c_void_p, C.c_void_p, C.POINTER(RayFrame)]; f.restype = C.c_int
    ce, d = np.ascontiguousarray(centre, dtype=np.float64).reshape(3), np.ascontiguousarray(delta, dtype=np.float64).reshape(6)
    out = RayFrame()
    rc = f(C.byref(frame), _ptr(ce), _ptr(d), C.byref(out))
    if rc != 0:
        raise RuntimeError(f"immesh_align_update failed rc={rc}")
    return out


class TopologyStats(C.Structure):
    """immesh_topology_stats (include/immesh_topology.h): the counts of the last analysis of the caster's snapshot"""
    _fields_ = [(n, C.c_int64) for n in ("n_faces", "n_counting", "n_degenerate", "n_vertices_used", "n_edges", "n_boundary", "n_interior", "n_nonmanifold",
                                         "n_inconsistent", "n_components", "largest_component_faces", "n_boundary_loops", "largest_loop_edges", "euler")]


assert C.sizeof(TopologyStats) == 112
EDGE_BOUNDARY, EDGE_NONMANIFOLD, EDGE_INCONSISTENT = 0, 1, 2
E_INTERNAL = -8


class OrientStats(C.Structure):
    """immesh_orient_stats (include/immesh_topology.h): the counts of the last orientation of the analysed snapshot"""
    _fields_ = [(n, C.c_int64) for n in ("n_patches", "n_orientable", "n_nonorientable", "largest_patch_faces", "n_faces_flipped", "n_faces_nonorientable",
                                         "n_patches_inverted", "n_inconsistent_before", "n_inconsistent_after")]


assert C.sizeof(OrientStats) == 72
ORIENT_FIRST, ORIENT_FEWEST, ORIENT_VIEWPOINT = 0, 1, 2
NORMALS_CANONICAL, NORMALS_VIEWPOINT = 0, 1                                          # include/immesh_normals.h: the sign of a cloud normal


class HolesStats(C.Structure):
    """immesh_holes_stats (include/immesh_topology.h): the counts of the last holes pass over the analysed snapshot"""
    _fields_ = [(n, C.c_int64) for n in ("n_loops", "n_simple", "n_nonsimple", "n_outline", "n_too_long", "n_too_wide", "n_blocked", "n_filled",
                                         "n_new_faces", "n_edges_closed", "largest_simple_loop_edges", "n_cycle_vertices")]


assert C.sizeof(HolesStats) == 96
HOLE_FILLED, HOLE_NONSIMPLE, HOLE_OUTLINE, HOLE_TOO_LONG, HOLE_TOO_WIDE, HOLE_BLOCKED = 0, 1, 2, 3, 4, 5


class ManifoldStats(C.Structure):
    """immesh_manifold_stats (include/immesh_topology.h): the counts of the last manifold pass over the analysed snapshot"""
    _fields_ = [(n, C.c_int64) for n in ("n_corners", "n_fans", "n_vertices_used", "n_singular_vertices", "most_fans_at_vertex", "n_new_vertices",
                                         "n_corners_moved", "n_faces_changed", "n_closed_fans", "n_open_fans", "largest_fan_corners",
                                         "n_nonmanifold_before")]


assert C.sizeof(ManifoldStats) == 96


class SimplifyStats(C.Structure):
    """immesh_simplify_stats (include/immesh_simplify.h): the counts of the last weld / clustering pass over the caster's snapshot"""
    _fields_ = [(n, C.c_int64) for n in ("n_vertices_in", "n_vertices_used", "n_alone_not_finite", "n_alone_outside", "n_vertices_out", "largest_cluster",
                                         "n_faces_in", "n_not_counting", "n_collapsed", "n_duplicate", "n_faces_out")]


assert C.sizeof(SimplifyStats) == 88
SIMPLIFY_FIRST, SIMPLIFY_MEAN = 0, 1
FACE_KEPT, FACE_NOT_COUNTING, FACE_COLLAPSED, FACE_DUPLICATE = 0, 1, 2, 3


class SmoothStats(C.Structure):
    """immesh_smooth_stats (include/immesh_smooth.h): the counts of the last smoothing pass over the caster's snapshot"""
    _fields_ = [(n, C.c_int64) for n in ("n_vertices", "n_used", "n_not_finite", "n_border", "n_interior", "n_moving", "n_pairs", "max_valence", "n_steps",
                                         "n_held", "n_moved")] + [("max_disp2", C.c_double)]


assert C.sizeof(SmoothStats) == 96
VERTEX_UNUSED, VERTEX_NOT_FINITE, VERTEX_BORDER, VERTEX_INTERIOR = 0, 1, 2, 3
SMOOTH_BORDER_FIXED, SMOOTH_BORDER_ALONG, SMOOTH_BORDER_FREE = 0, 1, 2


class IntersectStats(C.Structure):
    """immesh_intersect_stats (include/immesh_intersect.h): the counts of the last self-intersection pass over the caster's snapshot"""
    _fields_ = [(n, C.c_int64) for n in ("n_faces", "n_in_tree", "n_taking_part", "n_candidates")] + [("n_share", C.c_int64 * 4)] + \
               [(n, C.c_int64) for n in ("n_pairs", "n_pairs_share0", "n_pairs_share1", "n_faces_hit", "max_partners")]


assert C.sizeof(IntersectStats) == 104


class Image(C.Structure):
    """immesh_image (include/immesh_colour.h): one camera frame, its intrinsics, pose, exposure and gates"""
    _fields_ = [("data", C.c_void_p), ("rows", C.c_int32), ("cols", C.c_int32), ("row_stride_bytes", C.c_int64),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("rot", C.c_double * 9), ("pos", C.c_double * 3),
                ("fov_margin", C.c_double), ("inv_exposure", C.c_double), ("obs_time", C.c_double), ("min_depth", C.c_double), ("max_depth", C.c_double),
                ("max_pe_error", C.c_double)]


class ColourStats(C.Structure):
    """immesh_colour_stats"""
    _fields_ = [(n, C.c_int64) for n in ("n_set", "n_selected", "n_hit", "n_first", "n_updated", "pe_count")] + [("pe_sum", C.c_double), ("min_dis", C.c_double)]


COLOUR_STATE_DTYPE = np.dtype([("rgb", "<f8", 3), ("cov", "<f8", 3), ("first_exposure", "<f8"), ("obs_dis", "<f8"), ("last_obs_time", "<f8"),
                               ("n_obs", "<i4"), ("pad", "<i4")])   # immesh_colour_state
assert COLOUR_STATE_DTYPE.itemsize == 80 and C.sizeof(ColourStats) == 64 and C.sizeof(Image) == 200
COLOUR_PLAIN, COLOUR_VIEW = 0, 1
COLOUR_SET_ALL, COLOUR_SET_IDS, COLOUR_SET_RECENT, COLOUR_SET_RECENT_HEADS = 0, 1, 2, 3


def default_image(lib, pixels=None, **over):
    """immesh_default_image (identity pose, margin 0.005, inverse exposure 0.01, depths 3 / 200, pe 40) around `pixels` ((rows, cols, 3) uint8; the
    returned structure keeps it alive), fields overridden by keyword"""
    im = Image()
    lib.immesh_default_image.argtypes = [C.POINTER(Image)]; lib.immesh_default_image.restype = None
    lib.immesh_default_image(C.byref(im))
    if pixels is not None:
        px = np.asarray(pixels)
        if px.dtype != np.uint8 or px.ndim != 3 or px.shape[2] != 3 or px.strides[2] != 1 or px.strides[1] != 3:
            px = np.ascontiguousarray(px, dtype=np.uint8).reshape(px.shape[0], px.shape[1], 3)
        im._pixels = px
        im.data = px.ctypes.data; im.rows, im.cols = px.shape[:2]; im.row_stride_bytes = px.strides[0]
    for k, v in over.items():
        if k in ("rot", "pos"):
            getattr(im, k)[:] = [float(x) for x in np.asarray(v, float).reshape(-1)]
        else:
            setattr(im, k, v)
    return im


class Shade(C.Structure):
    """immesh_shade (include/immesh_shade.h): the colour pass behind a render"""
    _fields_ = [("source", C.c_int32), ("axis", C.c_int32), ("light", C.c_int32), ("bgr", C.c_int32), ("min_views", C.c_int32),
                ("background", C.c_uint8 * 3), ("pad", C.c_uint8), ("axis_min", C.c_double), ("axis_max", C.c_double)]


assert C.sizeof(Shade) == 40
SHADE_WHITE, SHADE_AXIS, SHADE_VERTEX = 0, 1, 2


def default_shade(lib, **over):
    """immesh_default_shade (WHITE, axis 2, light on, black background, range 0 / 0 = from the vertices) with fields overridden by keyword"""
    sh = Shade()
    lib.immesh_default_shade.argtypes = [C.POINTER(Shade)]; lib.immesh_default_shade.restype = None
    lib.immesh_default_shade(C.byref(sh))
    for k, v in over.items():
        if k == "background":
            sh.background[:] = [int(x) for x in v]
        else:
            setattr(sh, k, v)
    return sh


class RegionInfo(C.Structure):
    """immesh_region_info (include/immesh_regions.h): one region bucket of the renderer"""
    _fields_ = [("key", C.c_int32 * 3), ("index", C.c_int32), ("n_triangles", C.c_int32), ("dirty", C.c_int32), ("first", C.c_int64)]


REGION_DTYPE = np.dtype([("key", "<i4", 3), ("index", "<i4"), ("n_triangles", "<i4"), ("dirty", "<i4"), ("first", "<i8")])
assert REGION_DTYPE.itemsize == C.sizeof(RegionInfo) == 32


class Counters(C.Structure):
    _fields_ = [(n, C.c_int64) for n in COUNTER_FIELDS]


# -- checkpoints (include/immesh_checkpoint.h) ------------------------------------------------------------------------------------------------
E_INVAL, E_CAPACITY, E_IO, E_FORMAT = -1, -4, -6, -7
CHECKPOINT_VERSION = 1
CHECKPOINT_COUNT_FIELDS = ("n_root_voxels", "n_nodes", "n_point_chunks", "n_free_chunks", "n_ext_tables", "n_leaf_chunks", "n_vertices", "n_mesh_voxels",
                           "n_triangles_pool", "n_triangles_live", "n_adj_chunks", "n_regions", "scans_meshed", "map_updates")


class CheckpointSection(C.Structure):
    """immesh_checkpoint_section: one entry of a checkpoint's section table"""
    _fields_ = [("name", C.c_char * 24), ("offset", C.c_int64), ("bytes", C.c_int64), ("records", C.c_int64), ("checksum", C.c_uint64)]


class CheckpointInfo(C.Structure):
    """immesh_checkpoint_info"""
    _fields_ = ([("version", C.c_int32), ("n_sections", C.c_int32), ("has_regions", C.c_int32), ("has_colour", C.c_int32), ("file_bytes", C.c_int64), ("cfg", Config)] +
                [(n, C.c_int64) for n in CHECKPOINT_COUNT_FIELDS] + [("ms", C.c_float * 4)])


class CheckpointError(RuntimeError):
    """a refused checkpoint call: .rc is the IMMESH_E_* code, the text names the fault"""
    def __init__(self, what, rc, msg):
        super().__init__(f"{what} failed rc={rc}: {msg}")
        self.rc, self.msg = rc, msg


def _checkpoint_info_dict(info):
    out = {n: getattr(info, n) for n in ("version", "n_sections", "has_regions", "has_colour", "file_bytes") + CHECKPOINT_COUNT_FIELDS}
    out["cfg"] = info.cfg
    out["ms"] = tuple(float(v) for v in info.ms)
    return out


def checkpoint_probe(lib, path, cap=256):
    """immesh_checkpoint_probe (host only, needs no context) -> (info dict, [section dicts]); CheckpointError when the file is refused"""
    f = lib.immesh_checkpoint_probe
    f.argtypes = [C.c_char_p, C.POINTER(CheckpointInfo), C.POINTER(CheckpointSection), C.c_int32, C.c_char_p, C.c_int32]; f.restype = C.c_int
    info, secs, err = CheckpointInfo(), (CheckpointSection * cap)(), C.create_string_buffer(512)
    rc = f(os.fsencode(path), C.byref(info), secs, cap, err, len(err))
    if rc != 0:
        raise CheckpointError("immesh_checkpoint_probe", rc, err.value.decode())
    out = [{"name": s.name.decode(), "offset": s.offset, "bytes": s.bytes, "records": s.records, "checksum": s.checksum} for s in secs[:min(cap, info.n_sections)]]
    return _checkpoint_info_dict(info), out


def avia_config(**over):
    """config/avia.yaml + launch/mapping_avia.launch (SURVEY.md section 8 constants table)."""
    c = Config()
    c.voxel_size = 0.5; c.max_layer = 2
    for i in range(5):
        c.layer_init[i] = 5
    c.max_points_size = 100; c.planer_threshold = 0.01; c.dept_err = 0.02; c.beam_err = 0.05; c.calib_laser = 0
    c.sigma_num = 3.0; c.max_iter = 4
    for i, v in enumerate([1, 0, 0, 0, 1, 0, 0, 0, 1]):
        c.extR[i] = v
    for i, v in enumerate([0.04165, 0.02326, -0.0284]):
        c.extT[i] = v
    c.mesh_min_spacing = 0.1; c.mesh_voxel = 0.4; c.mesh_region = 10.0; c.mesh_append_budget = 10000
    c.device = 0
    for k, v in over.items():
        setattr(c, k, v)
    return c


def velodyne_config(**over):
    """config/velodyne.yaml + launch/mapping_velody64.launch (KITTI)."""
    c = avia_config()
    c.voxel_size = 3.0; c.max_layer = 4; c.max_points_size = 1000; c.dept_err = 0.04; c.beam_err = 0.1; c.calib_laser = 1
    c.max_iter = 3
    for i in range(3):
        c.extT[i] = 0.0
    c.mesh_min_spacing = 0.1 * 1.5; c.mesh_voxel = 0.4 * 1.5; c.mesh_region = 10.0 * 1.5; c.mesh_append_budget = 10000
    for k, v in over.items():
        setattr(c, k, v)
    return c


def make_state(R=None, t=None, cov_diag=1e-7, vel=None, gravity=None):
    """StatesGroup() defaults: identity pose, cov = I * INIT_COV (include/common_lib.h:201-210)."""
    s = np.zeros(STATE_DOUBLES)
    s[0:9] = (np.eye(3) if R is None else np.asarray(R, float)).reshape(-1)
    if t is not None:
        s[9:12] = t
    if vel is not None:
        s[12:15] = vel
    if gravity is not None:
        s[21:24] = gravity
    s[24:] = (np.eye(18) * cov_diag).reshape(-1)
    return s


class ImuSample(C.Structure):
    """immesh_imu_sample"""
    _fields_ = [("t", C.c_double), ("gyr", C.c_double * 3), ("acc", C.c_double * 3)]


class ImuCtx(C.Structure):
    """immesh_imu_ctx: the ImuProcess members UndistortPcl carries from scan to scan"""
    _fields_ = [("last_lidar_end_time", C.c_double), ("acc_s_last", C.c_double * 3), ("angvel_last", C.c_double * 3), ("last_imu", ImuSample),
                ("mean_acc_norm", C.c_double), ("cov_gyr", C.c_double * 3), ("cov_acc", C.c_double * 3), ("cov_bias_gyr", C.c_double * 3),
                ("cov_bias_acc", C.c_double * 3), ("lid_rot_to_imu", C.c_double * 9), ("lid_offset_to_imu", C.c_double * 3)]


def make_imu_ctx(cfg, t0=0.0, gyr0=(0, 0, 0), acc0=(0, 0, 9.81)):
    """ImuProcess after IMU_init (src/IMU_Processing.cpp:56-80, 186-230): noise parameters of config/avia.yaml, extrinsics of cfg."""
    ic = ImuCtx()
    ic.last_lidar_end_time = t0
    ic.last_imu.t = t0
    for a in range(3):
        ic.last_imu.gyr[a] = gyr0[a]; ic.last_imu.acc[a] = acc0[a]
        ic.cov_gyr[a] = 0.3; ic.cov_acc[a] = 0.5; ic.cov_bias_gyr[a] = 0.0001; ic.cov_bias_acc[a] = 0.0001
        ic.lid_offset_to_imu[a] = cfg.extT[a]
    ic.mean_acc_norm = float(np.linalg.norm(acc0))
    for i in range(9):
        ic.lid_rot_to_imu[i] = cfg.extR[i]
    return ic


def forward_without_imu_native(lib, state, dt=0.1, cov_gyr=0.3, cov_acc=0.5):
    """immesh_forward_without_imu (C++ host code in the product library); same arithmetic as synth.forward_without_imu."""
    f = lib.immesh_forward_without_imu
    f.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p]; f.restype = C.c_int
    out = np.empty(STATE_DOUBLES)
    s = np.ascontiguousarray(state, dtype=np.float64)
    if f(s.ctypes.data_as(C.c_void_p), dt, cov_gyr, cov_acc, out.ctypes.data_as(C.c_void_p)) != 0:
        raise RuntimeError("immesh_forward_without_imu failed")
    return out


def shard_owner(lib, cfg, key3):
    f = lib.immesh_shard_owner; f.argtypes = [C.POINTER(Config), C.c_void_p]; f.restype = C.c_int
    k = np.ascontiguousarray(key3, dtype=np.int64)
    return f(C.byref(cfg), k.ctypes.data_as(C.c_void_p))


def hip_library_path():
    # IMMESH_HIP_LIBRARY: an A/B measurement against a library built from another commit (tools/r06_ab.sh); never set by tests or the default bench
    return os.environ.get("IMMESH_HIP_LIBRARY") or os.path.join(_HERE, "csrc", "libimmesh_hip.so")


def load_hip_library():
    """Load the product library.  Raises (never falls back) when it has not been built."""
    p = hip_library_path()
    if not os.path.exists(p):
        raise RuntimeError(f"{p} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (or make -C immesh_amd/csrc). "
                           "There is no CPU fallback for the hot path.")
    return C.CDLL(p)


def _ptr(a):
    """host ndarray or raw device pointer (int) -> c_void_p"""
    if a is None:
        return None
    if isinstance(a, (int, np.integer)):
        return C.c_void_p(int(a))
    return a.ctypes.data_as(C.c_void_p)


class HotPath:
    def __init__(self, lib, cfg, prefix="immesh_"):
        self.lib, self.prefix, self.cfg = lib, prefix, cfg
        self._f = lambda name: getattr(lib, prefix + name)
        cr = self._f("create"); cr.restype = C.c_void_p; cr.argtypes = [C.POINTER(Config)]
        self.ctx = cr(C.byref(cfg))
        if not self.ctx:
            msg = ""
            if prefix == "immesh_":
                lib.immesh_create_error.restype = C.c_char_p
                msg = lib.immesh_create_error().decode()
            raise RuntimeError(f"{prefix}create failed: {msg}")
        self.ctx = C.c_void_p(self.ctx)

    def close(self):
        if getattr(self, "_colourer", None):                 # the colourer goes before its context
            g = self.lib.immesh_colourer_destroy; g.argtypes = [C.c_void_p]; g.restype = None
            g(self._colourer)
            self._colourer = None
        if getattr(self, "_cloud_index", None):              # the cloud index goes before its context (and before the caster whose samples it reads)
            g = self.lib.immesh_cloud_index_destroy; g.argtypes = [C.c_void_p]; g.restype = None
            g(self._cloud_index)
            self._cloud_index = None
        if getattr(self, "_raycaster", None):                # the ray caster goes before its context
            g = self.lib.immesh_raycaster_destroy; g.argtypes = [C.c_void_p]; g.restype = None
            g(self._raycaster)
            self._raycaster = None
        if getattr(self, "_renderer", None):                 # the renderer goes before its context
            g = self.lib.immesh_renderer_destroy; g.argtypes = [C.c_void_p]; g.restype = None
            g(self._renderer)
            self._renderer = None
        if self.ctx:
            d = self._f("destroy"); d.argtypes = [C.c_void_p]; d.restype = None
            d(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = ""
            if self.prefix == "immesh_":
                f = self.lib.immesh_last_error; f.restype = C.c_char_p; f.argtypes = [C.c_void_p]
                msg = f(self.ctx).decode()
            raise RuntimeError(f"{self.prefix}{what} failed rc={rc}: {msg}")

    # -- registration ------------------------------------------------------------------------------------------
    def map_build(self, pts_body_xyz, state, n=None):
        f = self._f("map_build"); f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]; f.restype = C.c_int
        n = len(pts_body_xyz) if n is None else n
        self._check(f(self.ctx, _ptr(pts_body_xyz), n, _ptr(state)), "map_build")

    def register(self, pts_down, state_prior, state, n=None, want_eff=False):
        f = self._f("register"); f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        n = len(pts_down) if n is None else n
        out = np.array(state, dtype=np.float64, copy=True)
        n_iter, n_match, res = C.c_int32(0), C.c_int32(0), C.c_double(0)
        eff_p = np.zeros((n, 3), np.float32) if want_eff else None
        eff_n = np.zeros((n, 4), np.float32) if want_eff else None
        self._check(f(self.ctx, _ptr(pts_down), n, _ptr(np.ascontiguousarray(state_prior, dtype=np.float64)), _ptr(out), C.byref(n_iter),
                      C.byref(n_match), C.byref(res), _ptr(eff_p), _ptr(eff_n)), "register")
        info = {"n_iter": n_iter.value, "n_match": n_match.value, "res_mean": res.value}
        if want_eff:
            info["eff_pts"] = eff_p[:n_match.value]; info["eff_norm_dis"] = eff_n[:n_match.value]
        return out, info

    def residuals(self, pts_down, state, n=None):
        f = self._f("residuals"); f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p] + [C.c_void_p] * 7
        n = len(pts_down) if n is None else n
        HTH, HTz, nm = np.zeros(36), np.zeros(6), C.c_int32(0)
        idx, nrm, dis, rinv = np.zeros(n, np.int32), np.zeros((n, 3)), np.zeros(n, np.float32), np.zeros(n)
        self._check(f(self.ctx, _ptr(pts_down), n, _ptr(np.ascontiguousarray(state, dtype=np.float64)), _ptr(HTH), _ptr(HTz), C.byref(nm),
                      _ptr(idx), _ptr(nrm), _ptr(dis), _ptr(rinv)), "residuals")
        m = nm.value
        return {"HTH": HTH.reshape(6, 6), "HTz": HTz, "n_match": m, "match_idx": idx[:m], "normals": nrm[:m], "dis": dis[:m], "r_inv": rinv[:m]}

    def map_update(self, pts_down, state, n=None):
        f = self._f("map_update"); f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]; f.restype = C.c_int
        n = len(pts_down) if n is None else n
        self._check(f(self.ctx, _ptr(pts_down), n, _ptr(np.ascontiguousarray(state, dtype=np.float64))), "map_update")

    # -- meshing -----------------------------------------------------------------------------------------------
    def mesh_scan(self, pts_world_xyzi, sensor_pos, frame_idx=0, n=None, fetch=True):
        f = self._f("mesh_scan"); f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]; f.restype = C.c_int
        n = len(pts_world_xyzi) if n is None else n
        self._check(f(self.ctx, _ptr(pts_world_xyzi), n, _ptr(np.ascontiguousarray(sensor_pos, dtype=np.float64)), frame_idx), "mesh_scan")
        return self.mesh_fetch() if fetch else None

    def reconstruct_mesh_from_pointcloud(self, pts_xyzi, leaf=0.01):
        f = self._f("reconstruct_mesh_from_pointcloud"); f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_double]; f.restype = C.c_int
        self._check(f(self.ctx, _ptr(pts_xyzi), len(pts_xyzi), leaf), "reconstruct_mesh_from_pointcloud")
        return self.mesh_fetch()

    def reconstruct_mesh_from_pointcloud_dev(self, dev_ptr, n, leaf=0.01):
        """the offline entry on a device-resident (n x 4 float32) cloud; the result lists are not fetched"""
        f = self._f("reconstruct_mesh_from_pointcloud"); f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_double]; f.restype = C.c_int
        self._check(f(self.ctx, dev_ptr, n, leaf), "reconstruct_mesh_from_pointcloud")

    def mesh_neighbourhood_sizes(self):
        """n_u of every voxel the newest finished mesh job triangulated (diagnostics; HIP library only)."""
        f = self._f("mesh_neighbourhood_sizes"); f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]; f.restype = C.c_int
        n = C.c_int32(0)
        self._check(f(self.ctx, None, 0, C.byref(n)), "mesh_neighbourhood_sizes")
        out = np.zeros(max(1, n.value), np.int32)
        self._check(f(self.ctx, _ptr(out), len(out), C.byref(n)), "mesh_neighbourhood_sizes")
        return out[:n.value]

    def mesh_old_set_sizes(self):
        """per voxel of the last meshed scan, in the order of mesh_neighbourhood_sizes: the live triangles whose smallest vertex lies in the
        neighbourhood, i.e. what the device gathers from its smallest-vertex lists before the containment filter (oracle only: test introspection)."""
        if self.prefix != "orc_":
            raise RuntimeError("mesh_old_set_sizes is an introspection entry of the oracle; the product library has no such entry point")
        f = self._f("mesh_old_set_sizes"); f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]; f.restype = C.c_int
        n = C.c_int32(0)
        self._check(f(self.ctx, None, 0, C.byref(n)), "mesh_old_set_sizes")
        out = np.zeros(max(1, n.value), np.int32)
        self._check(f(self.ctx, _ptr(out), len(out), C.byref(n)), "mesh_old_set_sizes")
        return out[:n.value]

    def mesh_world_scan(self):
        """the world-frame scan (n x 4 float32) the newest finished mesh job was handed (parity diagnostics)"""
        f = self._f("mesh_world_scan"); f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]; f.restype = C.c_int
        n = C.c_int32(0)
        self._check(f(self.ctx, None, 0, C.byref(n)), "mesh_world_scan")
        out = np.zeros((n.value, 4), np.float32)
        if n.value:
            self._check(f(self.ctx, _ptr(out), n.value, C.byref(n)), "mesh_world_scan")
        return out

    def mesh_wait(self):
        f = self._f("mesh_wait"); f.argtypes = [C.c_void_p]; f.restype = C.c_int
        self._check(f(self.ctx), "mesh_wait")

    def mesh_fetch(self):
        fs = self._f("mesh_sizes"); fs.argtypes = [C.c_void_p, C.POINTER(MeshSizes)]; fs.restype = C.c_int
        s = MeshSizes()
        self._check(fs(self.ctx, C.byref(s)), "mesh_sizes")
        r = {"vtx_base": s.vtx_base, "n_voxels_meshed": s.n_voxels_meshed,
             "new_vtx": np.zeros((s.n_new_vtx, 3), np.float32), "tri_add": np.zeros((s.n_add, 3), np.int32), "flip_add": np.zeros(s.n_add, np.uint8),
             "tri_rem": np.zeros((s.n_rem, 3), np.int32), "tri_upd": np.zeros((s.n_upd, 3), np.int32), "flip_upd": np.zeros(s.n_upd, np.uint8),
             "smooth_ids": np.zeros(s.n_smooth, np.int32), "smooth_xyz": np.zeros((s.n_smooth, 3), np.float64)}
        ff = self._f("mesh_fetch"); ff.argtypes = [C.c_void_p] + [C.c_void_p] * 8; ff.restype = C.c_int
        self._check(ff(self.ctx, _ptr(r["new_vtx"]), _ptr(r["tri_add"]), _ptr(r["flip_add"]), _ptr(r["tri_rem"]), _ptr(r["tri_upd"]),
                       _ptr(r["flip_upd"]), _ptr(r["smooth_ids"]), _ptr(r["smooth_xyz"])), "mesh_fetch")
        return r

    # -- mesh export ------------------------------------------------------------------------------------------
    def mesh_export(self, smooth_factor=1.0, knn=20):
        f = self._f("mesh_export"); f.argtypes = [C.c_void_p, C.c_double, C.c_int32, C.c_void_p, C.c_void_p]; f.restype = C.c_int
        nv, nf = C.c_int64(0), C.c_int64(0)
        self._check(f(self.ctx, smooth_factor, knn, C.byref(nv), C.byref(nf)), "mesh_export")
        vtx, faces = np.zeros((nv.value, 3), np.float32), np.zeros((nf.value, 3), np.int32)
        g = self._f("mesh_export_fetch"); g.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]; g.restype = C.c_int
        self._check(g(self.ctx, _ptr(vtx), _ptr(faces)), "mesh_export_fetch")
        return vtx, faces

    def smooth_pts(self, ids, smooth_factor=1.0, knn=20, maximum_smooth_dis=0.0):
        """Global_map::smooth_pts for a batch of vertex ids -> (n, 3) float64"""
        f = self._f("smooth_pts"); f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_double, C.c_void_p]; f.restype = C.c_int
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        out = np.zeros((len(ids), 3), np.float64)
        self._check(f(self.ctx, _ptr(ids), len(ids), smooth_factor, knn, maximum_smooth_dis, _ptr(out)), "smooth_pts")
        return out

    def mesh_display_vertices(self, ids, smooth_factor=1.0, knn=20, maximum_smooth_dis=0.0):
        """get_pos(1) after the renderer's on-demand smoothing, as floats -> (n, 3) float32"""
        f = self._f("mesh_display_vertices"); f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_double, C.c_void_p]; f.restype = C.c_int
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        out = np.zeros((len(ids), 3), np.float32)
        self._check(f(self.ctx, _ptr(ids), len(ids), smooth_factor, knn, maximum_smooth_dis, _ptr(out)), "mesh_display_vertices")
        return out

    def save_ply(self, path, smooth_factor=1.0, knn=20):
        f = self._f("save_ply"); f.argtypes = [C.c_void_p, C.c_char_p, C.c_double, C.c_int32]; f.restype = C.c_int
        self._check(f(self.ctx, path.encode(), smooth_factor, knn), "save_ply")

    # -- the renderer's region buckets on the device (include/immesh_regions.h) -------------------------------------------------------------
    def _check_regions(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"immesh_{what} failed rc={rc}: {self.mesh_regions_error()}")

    def mesh_regions_error(self):
        f = self.lib.immesh_mesh_regions_error; f.argtypes = [C.c_void_p]; f.restype = C.c_char_p
        return f(self.ctx).decode()

    def mesh_regions_enable(self, on=True):
        """switch the device's region table on -- before the first mesh job of the context"""
        f = self.lib.immesh_mesh_regions_enable; f.argtypes = [C.c_void_p, C.c_int32]; f.restype = C.c_int
        self._check_regions(f(self.ctx, 1 if on else 0), "mesh_regions_enable")

    def mesh_regions(self):
        """the whole region table in index (creation) order -> structured array (REGION_DTYPE); flags untouched"""
        f = self.lib.immesh_mesh_regions; f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]; f.restype = C.c_int
        n = C.c_int32(0)
        self._check_regions(f(self.ctx, None, 0, C.byref(n)), "mesh_regions")
        out = np.zeros(n.value, REGION_DTYPE)
        if n.value:
            self._check_regions(f(self.ctx, _ptr(out), n.value, C.byref(n)), "mesh_regions")
        return out[:n.value]

    def mesh_regions_fetch(self, n_regions, n_triangles):
        """results of the last mesh_regions_sync -> {"regions" (REGION_DTYPE), "tri" (n, 3) int32, "flip" (n) uint8, "xyz" (n, 3, 3) float32}"""
        f = self.lib.immesh_mesh_regions_fetch; f.argtypes = [C.c_void_p] * 5; f.restype = C.c_int
        r = {"regions": np.zeros(n_regions, REGION_DTYPE), "tri": np.zeros((n_triangles, 3), np.int32), "flip": np.zeros(n_triangles, np.uint8),
             "xyz": np.zeros((n_triangles, 3, 3), np.float32)}
        self._check_regions(f(self.ctx, _ptr(r["regions"]), _ptr(r["tri"]), _ptr(r["flip"]), _ptr(r["xyz"])), "mesh_regions_fetch")
        return r

    def mesh_regions_sync(self, smooth_factor=1.0, knn=20, maximum_smooth_dis=0.0, force_all=False, fetch=True):
        """synchronize_triangle_list_for_disp on the device: the regions changed since the last sync (all with force_all), each with its live triangles
        (sorted triplets, flip bytes, nine display floats); region k's triangles are rows regions["first"][k] : + regions["n_triangles"][k]"""
        f = self.lib.immesh_mesh_regions_sync
        f.argtypes = [C.c_void_p, C.c_double, C.c_int32, C.c_double, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]; f.restype = C.c_int
        nr, nt = C.c_int32(0), C.c_int64(0)
        self._check_regions(f(self.ctx, smooth_factor, knn, maximum_smooth_dis, 1 if force_all else 0, C.byref(nr), C.byref(nt)), "mesh_regions_sync")
        return self.mesh_regions_fetch(nr.value, nt.value) if fetch else (nr.value, nt.value)

    def region_keys(self, vtx_xyz, tri):
        """immesh_region_keys: the key rule evaluated on the device for caller-supplied triangles -> (n, 3) int32"""
        f = self.lib.immesh_region_keys; f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]; f.restype = C.c_int
        vtx = np.ascontiguousarray(vtx_xyz, dtype=np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
        out = np.zeros((len(t), 3), np.int32)
        self._check_regions(f(self.ctx, _ptr(vtx), len(vtx), _ptr(t), len(t), _ptr(out)), "region_keys")
        return out

    # -- mesh depth images + LiDAR point reinforcement (include/immesh_render.h) --------------------------------------------------------------
    def renderer(self):
        """the context's renderer (created at first use, destroyed by close())"""
        if getattr(self, "_renderer", None) is None:
            f = self.lib.immesh_renderer_create; f.argtypes = [C.c_void_p]; f.restype = C.c_void_p
            r = f(self.ctx)
            if not r:
                self._check(-1, "renderer_create")
            self._renderer = C.c_void_p(r)
        return self._renderer

    def camera_from_state(self, state, cam=None):
        return camera_from_state(self.lib, state, cam)

    def default_depth_camera(self, **over):
        return default_depth_camera(self.lib, **over)

    def render_triangles(self, cam, vtx_xyz, faces, want_depth=True, want_face=True):
        """immesh_render_triangles on a host triangle soup -> (depth (h, w) float32 or None, face (h, w) int32 or None)"""
        f = self.lib.immesh_render_triangles
        f.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]; f.restype = C.c_int
        vtx = np.ascontiguousarray(vtx_xyz, dtype=np.float32).reshape(-1, 3)
        fc = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
        shape = (max(cam.height, 0), max(cam.width, 0))               # (a bad size is the library's to reject)
        depth = np.empty(shape, np.float32) if want_depth else None
        face = np.empty(shape, np.int32) if want_face else None
        self._check(f(self.renderer(), C.byref(cam), _ptr(vtx), len(vtx), _ptr(fc), len(fc), _ptr(depth), _ptr(face)), "render_triangles")
        return depth, face

    def render_mesh(self, cam, smooth_factor=1.0, knn=20, want_depth=True, want_face=True):
        """immesh_render_mesh: the live mesh as mesh_export(smooth_factor, knn) exports it -> (depth, face)"""
        f = self.lib.immesh_render_mesh
        f.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_double, C.c_int32, C.c_void_p, C.c_void_p]; f.restype = C.c_int
        shape = (max(cam.height, 0), max(cam.width, 0))
        depth = np.empty(shape, np.float32) if want_depth else None
        face = np.empty(shape, np.int32) if want_face else None
        self._check(f(self.renderer(), C.byref(cam), smooth_factor, knn, _ptr(depth), _ptr(face)), "render_mesh")
        return depth, face

    def render_points(self):
        """reinforced points of the last render, pixel order -> (n, 3) float32"""
        f = self.lib.immesh_render_points; f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]; f.restype = C.c_int
        n = C.c_int64(0)
        self._check(f(self.renderer(), None, 0, C.byref(n)), "render_points")
        out = np.zeros((n.value, 3), np.float32)
        self._check(f(self.renderer(), _ptr(out), n.value, C.byref(n)), "render_points")
        return out

    def render_timing(self):
        """device milliseconds of the last render: (rasterize, reinforce)"""
        f = self.lib.immesh_renderer_last_timing; f.argtypes = [C.c_void_p, C.c_void_p]; f.restype = C.c_int
        ms = (C.c_float * 2)()
        self._check(f(self.renderer(), ms), "renderer_last_timing")
        return float(ms[0]), float(ms[1])

    # -- rays cast at the mesh (include/immesh_raycast.h) ---------------------------------------------------------------------------------------
    def raycaster(self):
        """the context's ray caster (created at first use, destroyed by close())"""
        if getattr(self, "_raycaster", None) is None:
            f = self.lib.immesh_raycaster_create; f.argtypes = [C.c_void_p]; f.restype = C.c_void_p
            r = f(self.ctx)
            if not r:
                self._check(-1, "raycaster_create")
            self._raycaster = C.c_void_p(r)
        return self._raycaster

    def ray_frame_from_state(self, state):
        """immesh_ray_frame_from_state: the LiDAR frame of a pose (make_state layout) under the configuration's extrinsic -> RayFrame"""
        f = self.lib.immesh_ray_frame_from_state; f.argtypes = [C.POINTER(Config), C.c_void_p, C.POINTER(RayFrame)]; f.restype = C.c_int
        st = np.ascontiguousarray(state, dtype=np.float64)
        fr = RayFrame()
        rc = f(C.byref(self.cfg), _ptr(st), C.byref(fr))
        if rc != 0:
            raise RuntimeError(f"immesh_ray_frame_from_state failed rc={rc}")
        return fr

    def _raycast_sizes(self):
        f = self.lib.immesh_raycast_sizes; f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]; f.restype = C.c_int
        nv, nf, ni = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._check(f(self.raycaster(), C.byref(nv), C.byref(nf), C.byref(ni)), "raycast_sizes")
        return nv.value, nf.value, ni.value

    def raycast_build_triangles(self, vtx_xyz, faces):
        """immesh_raycast_build_triangles on a host triangle soup -> (n_vtx, n_faces, faces in the hierarchy)"""
        f = self.lib.immesh_raycast_build_triangles; f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]; f.restype = C.c_int
        vtx = np.ascontiguousarray(vtx_xyz, dtype=np.float32).reshape(-1, 3)
        fc = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
        self._check(f(self.raycaster(), _ptr(vtx), len(vtx), _ptr(fc), len(fc)), "raycast_build_triangles")
        return self._raycast_sizes()

    def raycast_build_mesh(self, smooth_factor=1.0, knn=20):
        """immesh_raycast_build_mesh: a snapshot of the live mesh as mesh_export(smooth_factor, knn) exports it -> (n_vtx, n_faces, faces in the hierarchy)"""
        f = self.lib.immesh_raycast_build_mesh; f.argtypes = [C.c_void_p, C.c_double, C.c_int32]; f.restype = C.c_int
        self._check(f(self.raycaster(), smooth_factor, knn), "raycast_build_mesh")
        return self._raycast_sizes()

    def raycast(self, frame, dirs, origins=None, t_min=0.0, t_max=200.0, mode=RAY_NEAREST, want_t=True, want_face=True):
        """immesh_raycast: dirs (n, 3) and origins (n, 3) or None, in the sensor frame -> (t (n,) float32 or None, face (n,) int32 or None); -1 = miss"""
        f = self.lib.immesh_raycast
        f.argtypes = [C.c_void_p, C.POINTER(RayFrame), C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_int32, C.c_void_p, C.c_void_p]
        f.restype = C.c_int
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        o = None if origins is None else np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        if o is not None and len(o) != len(d):
            raise ValueError("raycast: origins and dirs differ in length")
        t = np.empty(len(d), np.float32) if want_t else None
        face = np.empty(len(d), np.int32) if want_face else None
        self._check(f(self.raycaster(), C.byref(frame), _ptr(d), _ptr(o), len(d), t_min, t_max, mode, _ptr(t), _ptr(face)), "raycast")
        return t, face

    def raycast_points(self, downsample_res=0.01):
        """reinforced points of the last NEAREST cast, ray order -> (n, 3) float32"""
        f = self.lib.immesh_raycast_points; f.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_int64, C.c_void_p]; f.restype = C.c_int
        n = C.c_int64(0)
        self._check(f(self.raycaster(), downsample_res, None, 0, C.byref(n)), "raycast_points")
        out = np.zeros((n.value, 3), np.float32)
        self._check(f(self.raycaster(), downsample_res, _ptr(out), n.value, C.byref(n)), "raycast_points")
        return out

    def raycast_timing(self):
        """device milliseconds of the last (build, cast, reinforce)"""
        f = self.lib.immesh_raycaster_last_timing; f.argtypes = [C.c_void_p, C.c_void_p]; f.restype = C.c_int
        ms = (C.c_float * 3)()
        self._check(f(self.raycaster(), ms), "raycaster_last_timing")
        return float(ms[0]), float(ms[1]), float(ms[2])

    # -- point-to-mesh distances on the caster (include/immesh_closest.h) ---------------------------------------------------------------------------
    def closest_points(self, pts, max_dist, frame=None, want=("d2", "dist", "face", "xyz", "side")):
        """immesh_closest_points: pts (n, 3) in the world (frame None) or in the sensor frame -> dict of the wanted outputs: d2 (n,) float64,
        dist (n,) float32, face (n,) int32 (-1: none), xyz (n, 3) float32, side (n,) int8"""
        f = self.lib.immesh_closest_points
        f.argtypes = [C.c_void_p, C.POINTER(RayFrame), C.c_void_p, C.c_int64, C.c_double] + [C.c_void_p] * 5
        f.restype = C.c_int
        p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
        n = len(p)
        out = {"d2": np.empty(n, np.float64), "dist": np.empty(n, np.float32), "face": np.empty(n, np.int32), "xyz": np.empty((n, 3), np.float32),
               "side": np.empty(n, np.int8)}
        out = {k: v for k, v in out.items() if k in want}
        self._check(f(self.raycaster(), None if frame is None else C.byref(frame), _ptr(p), n, max_dist,
                      *[_ptr(out.get(k)) for k in ("d2", "dist", "face", "xyz", "side")]), "closest_points")
        return out

    def closest_stats(self, bin_width, n_bins):
        """immesh_closest_reduce over the caster's last query -> (ClosestStats, histogram (n_bins,) int64)"""
        f = self.lib.immesh_closest_reduce; f.argtypes = [C.c_void_p, C.c_double, C.c_int32, C.POINTER(ClosestStats), C.c_void_p]; f.restype = C.c_int
        st = ClosestStats()
        hist = np.zeros(max(int(n_bins), 0) if int(n_bins) <= (1 << 20) else 0, np.int64)      # (a bad size is the library's to reject)
        self._check(f(self.raycaster(), bin_width, n_bins, C.byref(st), _ptr(hist)), "closest_reduce")
        return st, hist

    def closest_timing(self):
        """device milliseconds of the last (query, reduction)"""
        f = self.lib.immesh_closest_last_timing; f.argtypes = [C.c_void_p, C.c_void_p]; f.restype = C.c_int
        ms = (C.c_float * 2)()
        self._check(f(self.raycaster(), ms), "closest_last_timing")
        return float(ms[0]), float(ms[1])

    # -- align a cloud to the caster's snapshot (include/immesh_align.h) -----------------------------------------------------------------------------
    def align_step(self, pts, opts, frame=None, want_face=False, want_terms=False):
        """immesh_align_step: one step at `frame` (None: world coordinates) -> (AlignSystem, face (n,) int32 or None, terms (n, 28) float64 or None)"""
        f = self.lib.immesh_align_step
        f.argtypes = [C.c_void_p, C.POINTER(RayFrame), C.c_void_p, C.c_int64, C.POINTER(AlignOptions), C.POINTER(AlignSystem), C.c_void_p, C.c_void_p]
        f.restype = C.c_int
        p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
        face = np.empty(len(p), np.int32) if want_face else None
        terms = np.empty((len(p), ALIGN_TERMS), np.float64) if want_terms else None
        sy = AlignSystem()
        self._check(f(self.raycaster(), None if frame is None else C.byref(frame), _ptr(p), len(p), C.byref(opts), C.byref(sy), _ptr(face), _ptr(terms)),
                    "align_step")
        return sy, face, terms

    def align_solve(self, system, damping=0.0):
        return align_solve(self.lib, system, damping)

    def align_update(self, frame, centre, delta):
        return align_update(self.lib, frame, centre, delta)

    def align(self, pts, opts=None, frame=None, centre=None, history_cap=None, **over):
        """immesh_align: the loop from `frame` (None: the identity) -> (AlignResult, history (iterations, 4) float64: n_used, rms, |omega|, |v|).
        opts: an AlignOptions, or None for align_options(**over); centre "mean": the mean of the finite points under `frame`, computed here in float64."""
        f = self.lib.immesh_align
        f.argtypes = [C.c_void_p, C.POINTER(RayFrame), C.c_void_p, C.c_int64, C.POINTER(AlignOptions), C.POINTER(AlignResult), C.c_void_p, C.c_int64]
        f.restype = C.c_int
        p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
        o = align_options(**over) if opts is None else opts
        if centre is not None:
            o = AlignOptions.from_buffer_copy(o)
            o.centre[:] = align_centre_mean(p, frame) if isinstance(centre, str) and centre == "mean" else [float(x) for x in centre]
        cap = max(0, min(int(o.max_iters), 10000)) if history_cap is None else history_cap
        hist = np.zeros((cap, 4), np.float64)
        res = AlignResult()
        self._check(f(self.raycaster(), None if frame is None else C.byref(frame), _ptr(p), len(p), C.byref(o), C.byref(res), _ptr(hist), cap), "align")
        return res, hist[:min(res.iterations, cap)]

    def align_timing(self):
        """device milliseconds of (the last step, the sum over the last loop's steps)"""
        f = self.lib.immesh_align_last_timing; f.argtypes = [C.c_void_p, C.c_void_p]; f.restype = C.c_int
        ms = (C.c_float * 2)()
        self._check(f(self.raycaster(), ms), "align_last_timing")
        return float(ms[0]), float(ms[1])

    def align_set_variant(self, variant):
        """immesh_align_set_variant: 0 the fused step (the default), 1 split, 2 fused without the register cap (for measurements; the same bits)"""
        f = self.lib.immesh_align_set_variant; f.argtypes = [C.c_void_p, C.c_int32]; f.restype = C.c_int
        self._check(f(self.raycaster(), variant), "align_set_variant")

    # -- align a cloud to the indexed cloud (include/immesh_align.h, the Cloud rule) ---------------------------------------------------------------------
    def align_cloud_step(self, pts, opts, huber=0.0, frame=None, want_index=False, want_terms=False):
        """immesh_align_cloud_step: one step at `frame` (None: world coordinates) against the index's cloud -> (AlignSystem, index (n,) int32 or None,
        terms (n, 28) float64 or None)"""
        f = self.lib.immesh_align_cloud_step
        f.argtypes = [C.c_void_p, C.POINTER(RayFrame), C.c_void_p, C.c_int64, C.POINTER(AlignOptions), C.c_double, C.POINTER(AlignSystem), C.c_void_p,
                      C.c_void_p]
        f.restype = C.c_int
        p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
        index = np.empty(len(p), np.int32) if want_index else None
        terms = np.empty((len(p), ALIGN_TERMS), np.float64) if want_terms else None
        sy = AlignSystem()
        self._check(f(self.cloud_index(), None if frame is None else C.byref(frame), _ptr(p), len(p), None if opts is None else C.byref(opts), huber,
                      C.byref(sy), _ptr(index), _ptr(terms)), "align_cloud_step")
        return sy, index, terms

    def align_cloud(self, pts, opts=None, huber=0.0, frame=None, centre=None, history_cap=None, **over):
        """immesh_align_cloud: the loop from `frame` (None: the identity) against the index's cloud -> (AlignResult, history (iterations, 4) float64:
        n_used, rms, |omega|, |v|).  opts, centre and history_cap as align()'s."""
        f = self.lib.immesh_align_cloud
        f.argtypes = [C.c_void_p, C.POINTER(RayFrame), C.c_void_p, C.c_int64, C.POINTER(AlignOptions), C.c_double, C.POINTER(AlignResult), C.c_void_p,
                      C.c_int64]
        f.restype = C.c_int
        p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
        o = align_options(**over) if opts is None else opts
        if centre is not None:
            o = AlignOptions.from_buffer_copy(o)
            o.centre[:] = align_centre_mean(p, frame) if isinstance(centre, str) and centre == "mean" else [float(x) for x in centre]
        cap = max(0, min(int(o.max_iters), 10000)) if history_cap is None else history_cap
        hist = np.zeros((max(cap, 0), 4), np.float64)
        res = AlignResult()
        self._check(f(self.cloud_index(), None if frame is None else C.byref(frame), _ptr(p), len(p), C.byref(o), huber, C.byref(res), _ptr(hist), cap),
                    "align_cloud")
        return res, hist[:min(res.iterations, max(cap, 0))]

    def align_cloud_timing(self):
        """device milliseconds of (the last step, the sum over the last loop's steps) of the Cloud rule"""
        f = self.lib.immesh_align_cloud_last_timing; f.argtypes = [C.c_void_p, C.c_void_p]; f.restype = C.c_int
        ms = (C.c_float * 2)()
        self._check(f(self.cloud_index(), ms), "align_cloud_last_timing")
        return float(ms[0]), float(ms[1])

    def align_cloud_set_variant(self, variant):
        """immesh_align_cloud_set_variant: 0 the fused step, 1 split (the default, by measurement); for measurements: the same bits"""
        f = self.lib.immesh_align_cloud_set_variant; f.argtypes = [C.c_void_p, C.c_int32]; f.restype = C.c_int
        self._check(f(self.cloud_index(), variant), "align_cloud_set_variant")

    # -- mesh-to-cloud distances (include/immesh_nearest.h) ------------------------------------------------------------------------------------------
    def cloud_index(self):
        """the context's cloud index (created at first use, destroyed by close())"""
        if getattr(self, "_cloud_index", None) is None:
            f = self.lib.immesh_cloud_index_create; f.argtypes = [C.c_void_p]; f.restype = C.c_void_p
            x = f(self.ctx)
            if not x:
                self._check(-1, "cloud_index_create")
            self._cloud_index = C.c_void_p(x)
        return self._cloud_index

    def cloud_index_build(self, xyz):
        """immesh_cloud_index_build on a host cloud (n, 3) -> (points given, points in the hierarchy)"""
        f = self.lib.immesh_cloud_index_build; f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]; f.restype = C.c_int
        p = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        self._check(f(self.cloud_index(), _ptr(p), len(p)), "cloud_index_build")
        g = self.lib.immesh_cloud_index_sizes; g.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]; g.restype = C.c_int
        n, ni = C.c_int64(0), C.c_int64(0)
        self._check(g(self.cloud_index(), C.byref(n), C.byref(ni)), "cloud_index_sizes")
        return n.value, ni.value

    def mesh_sample(self, density, seed=0, fetch=True):
        """immesh_mesh_sample on the caster's snapshot -> (xyz (n, 3) float32, face (n,) int32), or the count alone with fetch=False; the samples stay
        on the device for nearest_samples"""
        f = self.lib.immesh_mesh_sample
        f.argtypes = [C.c_void_p, C.c_double, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]; f.restype = C.c_int
        n = C.c_int64(0)
        self._check(f(self.raycaster(), density, seed, None, None, 0, C.byref(n)), "mesh_sample")
        if not fetch:
            return n.value
        xyz, face = np.zeros((n.value, 3), np.float32), np.zeros(n.value, np.int32)
        self._check(f(self.raycaster(), density, seed, _ptr(xyz), _ptr(face), n.value, C.byref(n)), "mesh_sample")
        return xyz, face

    def mesh_sample_timing(self):
        """device milliseconds of the last sampling (counts, scan + emit)"""
        f = self.lib.immesh_mesh_sample_last_timing; f.argtypes = [C.c_void_p, C.c_void_p]; f.restype = C.c_int
        ms = (C.c_float * 2)()
        self._check(f(self.raycaster(), ms), "mesh_sample_last_timing")
        return float(ms[0]), float(ms[1])

    def _nearest_outputs(self, n, want):
        out = {"d2": np.empty(n, np.float64), "dist": np.empty(n, np.float32), "index": np.empty(n, np.int32), "xyz": np.empty((n, 3), np.float32)}
        return {k: v for k, v in out.items() if k in want}

    def nearest_points(self, pts, max_dist, frame=None, want=("d2", "dist", "index", "xyz")):
        """immesh_nearest_points: pts (n, 3) in the world (frame None) or in the sensor frame -> dict of the wanted outputs: d2 (n,) float64,
        dist (n,) float32, index (n,) int32 (-1: none), xyz (n, 3) float32"""
        f = self.lib.immesh_nearest_points
        f.argtypes = [C.c_void_p, C.POINTER(RayFrame), C.c_void_p, C.c_int64, C.c_double] + [C.c_void_p] * 4
        f.restype = C.c_int
        p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
        out = self._nearest_outputs(len(p), want)
        self._check(f(self.cloud_index(), None if frame is None else C.byref(frame), _ptr(p), len(p), max_dist,
                      *[_ptr(out.get(k)) for k in ("d2", "dist", "index", "xyz")]), "nearest_points")
        return out

    def nearest_samples(self, max_dist, want=("d2", "dist", "index", "xyz")):
        """immesh_nearest_samples: the caster's last samples against the index, without a round trip -> the dict of nearest_points"""
        f = self.lib.immesh_nearest_samples; f.argtypes = [C.c_void_p, C.c_void_p, C.c_double] + [C.c_void_p] * 4; f.restype = C.c_int
        g = self.lib.immesh_mesh_sample_count; g.argtypes = [C.c_void_p, C.c_void_p]; g.restype = C.c_int
        n = C.c_int64(0)
        self._check(g(self.raycaster(), C.byref(n)), "mesh_sample_count")
        n = n.value
        out = self._nearest_outputs(n, want)
        self._check(f(self.cloud_index(), self.raycaster(), max_dist, *[_ptr(out.get(k)) for k in ("d2", "dist", "index", "xyz")]), "nearest_samples")
        return out

    def nearest_stats(self, bin_width, n_bins):
        """immesh_nearest_reduce over the index's last query -> (ClosestStats, histogram (n_bins,) int64); n_with_face reads: with a neighbour"""
        f = self.lib.immesh_nearest_reduce; f.argtypes = [C.c_void_p, C.c_double, C.c_int32, C.POINTER(ClosestStats), C.c_void_p]; f.restype = C.c_int
        st = ClosestStats()
        hist = np.zeros(max(int(n_bins), 0) if int(n_bins) <= (1 << 20) else 0, np.int64)      # (a bad size is the library's to reject)
        self._check(f(self.cloud_index(), bin_width, n_bins, C.byref(st), _ptr(hist)), "nearest_reduce")
        return st, hist

    def nearest_timing(self):
        """device milliseconds of the last (build, query, reduction)"""
        f = self.lib.immesh_nearest_last_timing; f.argtypes = [C.c_void_p, C.c_void_p]; f.restype = C.c_int
        ms = (C.c_float * 3)()
        self._check(f(self.cloud_index(), ms), "nearest_last_timing")
        return float(ms[0]), float(ms[1]), float(ms[2])

    # -- k nearest neighbours, radius counts, outlier removal on the cloud index (include/immesh_nearest.h) -------------------------------------------
    def _cloud_index_given(self):
        g = self.lib.immesh_cloud_index_sizes; g.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]; g.restype = C.c_int
        n = C.c_int64(0)
        self._check(g(self.cloud_index(), C.byref(n), None), "cloud_index_sizes")
        return n.value

    def _knn_outputs(self, n, k, want):
        kk = max(int(k), 0) if int(k) <= 64 else 0                                   # (a bad k is the library's to reject)
        out = {"count": np.empty(n, np.int32), "index": np.empty((n, kk), np.int32), "d2": np.empty((n, kk), np.float64), "mean": np.empty(n, np.float64)}
        return {key: v for key, v in out.items() if key in want}

    def knn_points(self, pts, k, max_dist, frame=None, want=("count", "index", "d2")):
        """immesh_knn_points: pts (n, 3) in the world (frame None) or in the sensor frame -> dict of the wanted outputs: count (n,) int32,
        index (n, k) int32 and d2 (n, k) float64, ascending in (d2, index), -1 in the slots past count"""
        f = self.lib.immesh_knn_points
        f.argtypes = [C.c_void_p, C.POINTER(RayFrame), C.c_void_p, C.c_int64, C.c_int32, C.c_double] + [C.c_void_p] * 3; f.restype = C.c_int
        p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
        out = self._knn_outputs(len(p), k, [w for w in want if w != "mean"])
        self._check(f(self.cloud_index(), None if frame is None else C.byref(frame), _ptr(p), len(p), k, max_dist,
                      *[_ptr(out.get(key)) for key in ("count", "index", "d2")]), "knn_points")
        return out

    def knn_cloud(self, k, max_dist, want=("count", "index", "d2", "mean")):
        """immesh_knn_cloud: every point of the index's cloud against the others -> the dict of knn_points and mean (n,) float64 (-1: no neighbour);
        without index and d2 the lists are not stored on the device"""
        f = self.lib.immesh_knn_cloud; f.argtypes = [C.c_void_p, C.c_int32, C.c_double] + [C.c_void_p] * 4; f.restype = C.c_int
        out = self._knn_outputs(self._cloud_index_given(), k, want)
        self._check(f(self.cloud_index(), k, max_dist, *[_ptr(out.get(key)) for key in ("count", "index", "d2", "mean")]), "knn_cloud")
        return out

    def radius_count_points(self, pts, radius, frame=None):
        """immesh_radius_count_points -> (n,) int32: the cloud points within radius of every query"""
        f = self.lib.immesh_radius_count_points
        f.argtypes = [C.c_void_p, C.POINTER(RayFrame), C.c_void_p, C.c_int64, C.c_double, C.c_void_p]; f.restype = C.c_int
        p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
        count = np.empty(len(p), np.int32)
        self._check(f(self.cloud_index(), None if frame is None else C.byref(frame), _ptr(p), len(p), radius, _ptr(count)), "radius_count_points")
        return count

    def radius_count_cloud(self, radius):
        """immesh_radius_count_cloud -> (n,) int32: the other cloud points within radius of every cloud point"""
        f = self.lib.immesh_radius_count_cloud; f.argtypes = [C.c_void_p, C.c_double, C.c_void_p]; f.restype = C.c_int
        count = np.empty(self._cloud_index_given(), np.int32)
        self._check(f(self.cloud_index(), radius, _ptr(count)), "radius_count_cloud")
        return count

    @staticmethod
    def _outlier_counts(counts):
        return dict(zip(("kept", "outliers", "isolated", "not_finite"), (int(v) for v in counts)))

    def cloud_outliers_statistical(self, mult):
        """immesh_cloud_outliers_statistical over the last knn_cloud -> dict: mu, sigma, threshold, kept, outliers, isolated, not_finite, keep (n,) bool"""
        f = self.lib.immesh_cloud_outliers_statistical; f.argtypes = [C.c_void_p, C.c_double] + [C.c_void_p] * 5; f.restype = C.c_int
        mu, sigma, thr = C.c_double(0), C.c_double(0), C.c_double(0)
        counts = np.zeros(4, np.int64)
        keep = np.zeros(self._cloud_index_given(), np.uint8)
        self._check(f(self.cloud_index(), mult, C.byref(mu), C.byref(sigma), C.byref(thr), _ptr(counts), _ptr(keep)), "cloud_outliers_statistical")
        return dict(mu=mu.value, sigma=sigma.value, threshold=thr.value, keep=keep.astype(bool), **self._outlier_counts(counts))

    def cloud_outliers_radius(self, min_neighbours):
        """immesh_cloud_outliers_radius over the last radius_count_cloud -> dict: kept, outliers, isolated, not_finite, keep (n,) bool"""
        f = self.lib.immesh_cloud_outliers_radius; f.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]; f.restype = C.c_int
        counts = np.zeros(4, np.int64)
        keep = np.zeros(self._cloud_index_given(), np.uint8)
        self._check(f(self.cloud_index(), min_neighbours, _ptr(counts), _ptr(keep)), "cloud_outliers_radius")
        return dict(keep=keep.astype(bool), **self._outlier_counts(counts))

    def cloud_index_apply_outliers(self):
        """immesh_cloud_index_apply_outliers: the kept points of the last mask become the index's cloud -> their old indices (n_kept,) int32"""
        f = self.lib.immesh_cloud_index_apply_outliers; f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]; f.restype = C.c_int
        kept = np.empty(self._cloud_index_given(), np.int32)                          # at most every point is kept
        n = C.c_int64(0)
        self._check(f(self.cloud_index(), _ptr(kept), len(kept), C.byref(n)), "cloud_index_apply_outliers")
        return kept[:n.value].copy()

    def cloud_index_points(self):
        """immesh_cloud_index_points: the index's cloud as it lies on the device -> (n, 3) float32"""
        f = self.lib.immesh_cloud_index_points; f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]; f.restype = C.c_int
        xyz = np.empty((self._cloud_index_given(), 3), np.float32)
        n = C.c_int64(0)
        self._check(f(self.cloud_index(), _ptr(xyz), len(xyz), C.byref(n)), "cloud_index_points")
        return xyz

    def knn_timing(self):
        """device milliseconds of the last (traversal of a neighbours / count query, mask, apply)"""
        f = self.lib.immesh_knn_last_timing; f.argtypes = [C.c_void_p, C.c_void_p]; f.restype = C.c_int
        ms = (C.c_float * 3)()
        self._check(f(self.cloud_index(), ms), "knn_last_timing")
        return float(ms[0]), float(ms[1]), float(ms[2])

    # -- Euclidean clusters of the cloud index (include/immesh_nearest.h, the Clusters rule) ----------------------------------------------------------
    def cloud_clusters(self, radius, min_neighbours=0, want=("label", "kind")):
        """immesh_cloud_clusters: DBSCAN over the index's cloud -> dict of the wanted outputs: label (n,) int32 (the cluster's number, -1: noise or not
        finite), kind (n,) uint8 (0 core, 1 border, 2 noise, 3 not finite), and always counts (core, border, noise, not_finite as a dict) and
        n_clusters; the clusters stay on the device for cloud_clusters_table and cloud_clusters_select"""
        f = self.lib.immesh_cloud_clusters; f.argtypes = [C.c_void_p, C.c_double, C.c_int64] + [C.c_void_p] * 4; f.restype = C.c_int
        n = self._cloud_index_given()
        out = {key: v for key, v in (("label", np.empty(n, np.int32)), ("kind", np.empty(n, np.uint8))) if key in want}
        counts, nc = np.zeros(4, np.int64), C.c_int64(0)
        self._check(f(self.cloud_index(), radius, min_neighbours, _ptr(out.get("label")), _ptr(out.get("kind")), _ptr(counts), C.byref(nc)), "cloud_clusters")
        out["counts"] = dict(zip(("core", "border", "noise", "not_finite"), (int(v) for v in counts)))
        out["n_clusters"] = nc.value
        return out

    def cloud_clusters_table(self):
        """immesh_cloud_clusters_table -> dict: first, n_points, n_core (n_clusters,) int32, box (n_clusters, 6) float32 (lo xyz, hi xyz)"""
        f = self.lib.immesh_cloud_clusters_table; f.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p]; f.restype = C.c_int
        n = C.c_int64(0)
        self._check(f(self.cloud_index(), None, None, None, None, 0, C.byref(n)), "cloud_clusters_table")
        n = n.value
        out = dict(first=np.empty(n, np.int32), n_points=np.empty(n, np.int32), n_core=np.empty(n, np.int32), box=np.empty((n, 6), np.float32))
        self._check(f(self.cloud_index(), _ptr(out["first"]), _ptr(out["n_points"]), _ptr(out["n_core"]), _ptr(out["box"]), n, None), "cloud_clusters_table")
        return out

    def cloud_clusters_select(self, min_points=0, max_points=0, keep_largest=0, keep_noise=False):
        """immesh_cloud_clusters_select over the last cloud_clusters -> dict: kept, dropped (in a cluster and not kept), noise (and not kept),
        not_finite, keep (n,) bool; the mask is the index's last mask, for cloud_index_apply_outliers"""
        f = self.lib.immesh_cloud_clusters_select; f.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]; f.restype = C.c_int
        counts = np.zeros(4, np.int64)
        keep = np.zeros(self._cloud_index_given(), np.uint8)
        self._check(f(self.cloud_index(), min_points, max_points, keep_largest, 1 if keep_noise else 0, _ptr(counts), _ptr(keep)), "cloud_clusters_select")
        return dict(keep=keep.astype(bool), **dict(zip(("kept", "dropped", "noise", "not_finite"), (int(v) for v in counts))))

    def clusters_timing(self):
        """device milliseconds of the last cloud_clusters (count and kinds, joins, border walk, numbering and table)"""
        f = self.lib.immesh_cloud_clusters_last_timing; f.argtypes = [C.c_void_p, C.c_void_p]; f.restype = C.c_int
        ms = (C.c_float * 4)()
        self._check(f(self.cloud_index(), ms), "cloud_clusters_last_timing")
        return tuple(float(v) for v in ms)

    # -- normals of the cloud and their agreement with the mesh (include/immesh_normals.h) ------------------------------------------------------------
    @staticmethod
    def _pair_counts(counts):
        return dict(zip(("pairs", "opposed", "no_pair", "not_finite"), (int(v) for v in counts)))

    def cloud_normals(self, k, max_dist, min_ratio=0.0, mode=NORMALS_CANONICAL, viewpoint=None, want=("normal", "curvature", "eig", "count", "status")):
        """immesh_cloud_normals: a normal per point of the index's cloud from its k nearest neighbours -> dict of the wanted outputs: normal (n, 3)
        float32 (NaN without one), curvature (n,) float64, eig (n, 3) float64 (smallest, middle, largest), count (n,) int32, status (n,) uint8
        (0 a normal, 1 too few neighbours, 3 line-like, 2 not finite), and always with_normal, too_few, line_like, not_finite; the normals stay on
        the device for the agreement calls"""
        f = self.lib.immesh_cloud_normals
        f.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_int32] + [C.c_void_p] * 7; f.restype = C.c_int
        n = self._cloud_index_given()
        out = {"normal": np.empty((n, 3), np.float32), "curvature": np.empty(n, np.float64), "eig": np.empty((n, 3), np.float64),
               "count": np.empty(n, np.int32), "status": np.empty(n, np.uint8)}
        out = {key: v for key, v in out.items() if key in want}
        vp = None if viewpoint is None else np.ascontiguousarray(viewpoint, dtype=np.float64).reshape(3)
        counts = np.zeros(4, np.int64)
        self._check(f(self.cloud_index(), k, max_dist, min_ratio, mode, _ptr(vp), *[_ptr(out.get(key)) for key in ("normal", "curvature", "eig", "count", "status")],
                      _ptr(counts)), "cloud_normals")
        out.update(zip(("with_normal", "too_few", "line_like", "not_finite"), (int(v) for v in counts)))
        return out

    def cloud_normals_get(self):
        """immesh_cloud_normals_get: the last normals as they lie on the device -> (normal (n, 3) float32, status (n,) uint8)"""
        f = self.lib.immesh_cloud_normals_get; f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]; f.restype = C.c_int
        n = C.c_int64(0)
        self._check(f(self.cloud_index(), None, None, 0, C.byref(n)), "cloud_normals_get")
        normal, status = np.empty((n.value, 3), np.float32), np.empty(n.value, np.uint8)
        self._check(f(self.cloud_index(), _ptr(normal), _ptr(status), n.value, C.byref(n)), "cloud_normals_get")
        return normal, status

    def normals_agree_samples(self, fetch=True):
        """immesh_normals_agree_samples: the face normal of every sample of the caster against the normal of its nearest cloud point (the last
        nearest_samples) -> dict: agree (n,) float32 (NaN without a pair; with fetch), pairs, opposed, no_pair, not_finite"""
        f = self.lib.immesh_normals_agree_samples; f.argtypes = [C.c_void_p] * 4; f.restype = C.c_int
        agree = None
        if fetch:
            g = self.lib.immesh_mesh_sample_count; g.argtypes = [C.c_void_p, C.c_void_p]; g.restype = C.c_int
            n = C.c_int64(0)
            self._check(g(self.raycaster(), C.byref(n)), "mesh_sample_count")
            agree = np.empty(n.value, np.float32)
        counts = np.zeros(4, np.int64)
        self._check(f(self.cloud_index(), self.raycaster(), _ptr(agree), _ptr(counts)), "normals_agree_samples")
        return dict({"agree": agree} if fetch else {}, **self._pair_counts(counts))

    def normals_agree_cloud(self, max_dist, fetch=True):
        """immesh_normals_agree_cloud: the normal of every cloud point against the normal of its closest face within max_dist -> dict: agree (n,)
        float32 and face (n,) int32 (with fetch), pairs, opposed, no_pair, not_finite"""
        f = self.lib.immesh_normals_agree_cloud; f.argtypes = [C.c_void_p, C.c_void_p, C.c_double] + [C.c_void_p] * 3; f.restype = C.c_int
        n = self._cloud_index_given()
        agree, face = (np.empty(n, np.float32), np.empty(n, np.int32)) if fetch else (None, None)
        counts = np.zeros(4, np.int64)
        self._check(f(self.cloud_index(), self.raycaster(), max_dist, _ptr(agree), _ptr(face), _ptr(counts)), "normals_agree_cloud")
        return dict({"agree": agree, "face": face} if fetch else {}, **self._pair_counts(counts))

    def normals_agree_stats(self, bin_width, n_bins):
        """immesh_normals_agree_reduce over the index's last agreement -> (ClosestStats, histogram (n_bins,) int64); n_with_face reads: pairs, and
        mean is the normal consistency"""
        f = self.lib.immesh_normals_agree_reduce; f.argtypes = [C.c_void_p, C.c_double, C.c_int32, C.POINTER(ClosestStats), C.c_void_p]; f.restype = C.c_int
        st = ClosestStats()
        hist = np.zeros(max(int(n_bins), 0) if int(n_bins) <= (1 << 20) else 0, np.int64)      # (a bad size is the library's to reject)
        self._check(f(self.cloud_index(), bin_width, n_bins, C.byref(st), _ptr(hist)), "normals_agree_reduce")
        return st, hist

    def normals_timing(self):
        """device milliseconds of the last (normals launch, agreement launch, reduction)"""
        f = self.lib.immesh_normals_last_timing; f.argtypes = [C.c_void_p, C.c_void_p]; f.restype = C.c_int
        ms = (C.c_float * 3)()
        self._check(f(self.cloud_index(), ms), "normals_last_timing")
        return float(ms[0]), float(ms[1]), float(ms[2])

    # -- the topology of the caster's snapshot (include/immesh_topology.h) ----------------------------------------------------------------------------
    def topology_analyse(self):
        """immesh_topology_analyse on the caster's snapshot -> TopologyStats; the analysis stays on the device for the calls below"""
        f = self.lib.immesh_topology_analyse; f.argtypes = [C.c_void_p, C.POINTER(TopologyStats)]; f.restype = C.c_int
        st = TopologyStats()
        self._check(f(self.raycaster(), C.byref(st)), "topology_analyse")
        return st

    def topology_faces(self):
        """the component number of every face (-1: the face does not count) -> (n_faces,) int32"""
        f = self.lib.immesh_topology_faces; f.argtypes = [C.c_void_p, C.c_void_p]; f.restype = C.c_int
        self._check(f(self.raycaster(), None), "topology_faces")
        comp = np.empty(self._raycast_sizes()[1], np.int32)
        self._check(f(self.raycaster(), _ptr(comp)), "topology_faces")
        return comp

    def topology_components(self):
        """the component tables -> dict: first_face, n_faces, n_boundary (n,) int32, box (n, 6) float32 (lo xyz, hi xyz)"""
        f = self.lib.immesh_topology_components; f.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p]; f.restype = C.c_int
        n = C.c_int64(0)
        self._check(f(self.raycaster(), None, None, None, None, 0, C.byref(n)), "topology_components")
        out = {"first_face": np.empty(n.value, np.int32), "n_faces": np.empty(n.value, np.int32), "n_boundary": np.empty(n.value, np.int32),
               "box": np.empty((n.value, 6), np.float32)}
        self._check(f(self.raycaster(), *[_ptr(out[k]) for k in ("first_face", "n_faces", "n_boundary", "box")], n.value, C.byref(n)), "topology_components")
        return out

    def topology_edges(self, kind):
        """the edges of one kind (EDGE_BOUNDARY, EDGE_NONMANIFOLD, EDGE_INCONSISTENT), ascending -> (uv (n, 2) int32, uses (n,) int32)"""
        f = self.lib.immesh_topology_edges; f.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]; f.restype = C.c_int
        n = C.c_int64(0)
        self._check(f(self.raycaster(), kind, None, None, 0, C.byref(n)), "topology_edges")
        uv, uses = np.empty((n.value, 2), np.int32), np.empty(n.value, np.int32)
        self._check(f(self.raycaster(), kind, _ptr(uv), _ptr(uses), n.value, C.byref(n)), "topology_edges")
        return uv, uses

    def topology_select(self, min_faces=0, min_diagonal=0.0, keep_largest=0, cap=None):
        """immesh_topology_select -> (keep (n_faces,) int8, the kept faces (n, 3) int32 in face order); cap: the room given for the kept faces (all by
        default)"""
        f = self.lib.immesh_topology_select
        f.argtypes = [C.c_void_p, C.c_int64, C.c_double, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]; f.restype = C.c_int
        n = C.c_int64(0)
        keep = np.empty(self._raycast_sizes()[1], np.int8)
        self._check(f(self.raycaster(), min_faces, min_diagonal, keep_largest, _ptr(keep), None, 0, C.byref(n)), "topology_select")
        cap = n.value if cap is None else cap
        out = np.empty((max(cap, 0), 3), np.int32)
        self._check(f(self.raycaster(), min_faces, min_diagonal, keep_largest, _ptr(keep), _ptr(out), cap, C.byref(n)), "topology_select")
        return keep, out[:n.value]

    def topology_timing(self):
        """device milliseconds of the last (analysis, select)"""
        f = self.lib.immesh_topology_last_timing; f.argtypes = [C.c_void_p, C.c_void_p]; f.restype = C.c_int
        ms = (C.c_float * 2)()
        self._check(f(self.raycaster(), ms), "topology_last_timing")
        return float(ms[0]), float(ms[1])

    def topology_orient(self, mode, viewpoint=None):
        """immesh_topology_orient on the analysed snapshot (ORIENT_FIRST, ORIENT_FEWEST, ORIENT_VIEWPOINT with viewpoint (3,)) -> OrientStats; the
        orientation stays on the device for the calls below"""
        f = self.lib.immesh_topology_orient; f.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(OrientStats)]; f.restype = C.c_int
        o = None if viewpoint is None else np.ascontiguousarray(viewpoint, dtype=np.float64).reshape(3)
        st = OrientStats()
        self._check(f(self.raycaster(), mode, _ptr(o), C.byref(st)), "topology_orient")
        return st

    def topology_orient_faces(self):
        """-> dict: patch (n_faces,) int32 (-1: the face does not count), flip (n_faces,) int8, faces (n_faces, 3) int32: every face, the flipped ones
        as (i0, i2, i1)"""
        f = self.lib.immesh_topology_orient_faces; f.argtypes = [C.c_void_p] + [C.c_void_p] * 3; f.restype = C.c_int
        self._check(f(self.raycaster(), None, None, None), "topology_orient_faces")
        nf = self._raycast_sizes()[1]
        out = {"patch": np.empty(nf, np.int32), "flip": np.empty(nf, np.int8), "faces": np.empty((nf, 3), np.int32)}
        self._check(f(self.raycaster(), _ptr(out["patch"]), _ptr(out["flip"]), _ptr(out["faces"])), "topology_orient_faces")
        return out

    def topology_orient_patches(self):
        """the patch tables -> dict: first_face, n_faces, orientable, n_flipped, n_inconsistent (n_patches,) int32"""
        f = self.lib.immesh_topology_orient_patches; f.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p]; f.restype = C.c_int
        n = C.c_int64(0)
        self._check(f(self.raycaster(), None, None, None, None, None, 0, C.byref(n)), "topology_orient_patches")
        names = ("first_face", "n_faces", "orientable", "n_flipped", "n_inconsistent")
        out = {k: np.empty(n.value, np.int32) for k in names}
        self._check(f(self.raycaster(), *[_ptr(out[k]) for k in names], n.value, C.byref(n)), "topology_orient_patches")
        return out

    def topology_orient_apply(self):
        """immesh_topology_orient_apply: the oriented faces become the caster's, on the device; the analysis and the orientation are discarded as by
        a build"""
        f = self.lib.immesh_topology_orient_apply; f.argtypes = [C.c_void_p]; f.restype = C.c_int
        self._check(f(self.raycaster()), "topology_orient_apply")

    def topology_orient_timing(self):
        """device milliseconds of the last (orient, apply)"""
        f = self.lib.immesh_topology_orient_last_timing; f.argtypes = [C.c_void_p, C.c_void_p]; f.restype = C.c_int
        ms = (C.c_float * 2)()
        self._check(f(self.raycaster(), ms), "topology_orient_last_timing")
        return float(ms[0]), float(ms[1])

    def topology_holes(self, max_edges, max_diagonal=0.0):
        """immesh_topology_holes on the analysed snapshot: the ordered cycles of the simple boundary loops, and fans over those of at most max_edges
        edges whose box diagonal is at most max_diagonal (0: any) -> HolesStats; the pass stays on the device for the calls below"""
        f = self.lib.immesh_topology_holes; f.argtypes = [C.c_void_p, C.c_int64, C.c_double, C.POINTER(HolesStats)]; f.restype = C.c_int
        st = HolesStats()
        self._check(f(self.raycaster(), max_edges, max_diagonal, C.byref(st)), "topology_holes")
        return st

    def topology_holes_loops(self):
        """the loop tables -> dict: first_vertex, n_edges, status (n_loops,) int32, box (n_loops, 6) float32, cycle_start (n_loops,) int64 (-1: the
        loop is not simple)"""
        f = self.lib.immesh_topology_holes_loops; f.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p]; f.restype = C.c_int
        n = C.c_int64(0)
        self._check(f(self.raycaster(), None, None, None, None, None, 0, C.byref(n)), "topology_holes_loops")
        out = {"first_vertex": np.empty(n.value, np.int32), "n_edges": np.empty(n.value, np.int32), "status": np.empty(n.value, np.int32),
               "box": np.empty((n.value, 6), np.float32), "cycle_start": np.empty(n.value, np.int64)}
        self._check(f(self.raycaster(), *[_ptr(out[k]) for k in ("first_vertex", "n_edges", "status", "box", "cycle_start")], n.value, C.byref(n)),
                    "topology_holes_loops")
        return out

    def topology_holes_cycles(self):
        """the boundary cycles in order: the simple loops' cycles concatenated in loop order -> (n_cycle_vertices,) int32"""
        f = self.lib.immesh_topology_holes_cycles; f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]; f.restype = C.c_int
        n = C.c_int64(0)
        self._check(f(self.raycaster(), None, 0, C.byref(n)), "topology_holes_cycles")
        out = np.empty(n.value, np.int32)
        self._check(f(self.raycaster(), _ptr(out), n.value, C.byref(n)), "topology_holes_cycles")
        return out

    def topology_holes_faces(self):
        """the fans -> (new_loop (n,) int32, new_faces (n, 3) int32)"""
        f = self.lib.immesh_topology_holes_faces; f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]; f.restype = C.c_int
        n = C.c_int64(0)
        self._check(f(self.raycaster(), None, None, 0, C.byref(n)), "topology_holes_faces")
        loop, faces = np.empty(n.value, np.int32), np.empty((n.value, 3), np.int32)
        self._check(f(self.raycaster(), _ptr(loop), _ptr(faces), n.value, C.byref(n)), "topology_holes_faces")
        return loop, faces

    def topology_holes_apply(self):
        """immesh_topology_holes_apply: faces ++ new_faces become the caster's, on the device, and its hierarchy is built again; everything a build
        discards is discarded"""
        f = self.lib.immesh_topology_holes_apply; f.argtypes = [C.c_void_p]; f.restype = C.c_int
        self._check(f(self.raycaster()), "topology_holes_apply")

    def topology_holes_timing(self):
        """device milliseconds of the last (holes pass, apply)"""
        f = self.lib.immesh_topology_holes_last_timing; f.argtypes = [C.c_void_p, C.c_void_p]; f.restype = C.c_int
        ms = (C.c_float * 2)()
        self._check(f(self.raycaster(), ms), "topology_holes_last_timing")
        return float(ms[0]), float(ms[1])

    def topology_manifold(self):
        """immesh_topology_manifold on the analysed snapshot: every fan of faces round a vertex gets a vertex of its own -> ManifoldStats; the pass
        stays on the device for the calls below"""
        f = self.lib.immesh_topology_manifold; f.argtypes = [C.c_void_p, C.POINTER(ManifoldStats)]; f.restype = C.c_int
        st = ManifoldStats()
        self._check(f(self.raycaster(), C.byref(st)), "topology_manifold")
        return st

    def topology_manifold_vertices(self):
        """-> n_fans_out (n_vtx,) int32: the fans at every vertex, 0 for an unused one"""
        f = self.lib.immesh_topology_manifold_vertices; f.argtypes = [C.c_void_p, C.c_void_p]; f.restype = C.c_int
        self._check(f(self.raycaster(), None), "topology_manifold_vertices")
        out = np.empty(self._raycast_sizes()[0], np.int32)
        self._check(f(self.raycaster(), _ptr(out)), "topology_manifold_vertices")
        return out

    def topology_manifold_fans(self):
        """the fan tables -> dict: vertex, first_face, n_corners, n_links, index_out (n_fans,) int32"""
        f = self.lib.immesh_topology_manifold_fans; f.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p]; f.restype = C.c_int
        n = C.c_int64(0)
        self._check(f(self.raycaster(), None, None, None, None, None, 0, C.byref(n)), "topology_manifold_fans")
        names = ("vertex", "first_face", "n_corners", "n_links", "index_out")
        out = {k: np.empty(n.value, np.int32) for k in names}
        self._check(f(self.raycaster(), *[_ptr(out[k]) for k in names], n.value, C.byref(n)), "topology_manifold_fans")
        return out

    def topology_manifold_faces(self):
        """-> (fan_out (n_faces, 3) int32, -1 for the corners of a face that does not count; faces_out (n_faces, 3) int32)"""
        f = self.lib.immesh_topology_manifold_faces; f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]; f.restype = C.c_int
        self._check(f(self.raycaster(), None, None), "topology_manifold_faces")
        nf = self._raycast_sizes()[1]
        fan, faces = np.empty((nf, 3), np.int32), np.empty((nf, 3), np.int32)
        self._check(f(self.raycaster(), _ptr(fan), _ptr(faces)), "topology_manifold_faces")
        return fan, faces

    def topology_manifold_new_vertices(self):
        """the new vertices -> (vsrc (n,) int32, xyz (n, 3) float32: the bits of their sources)"""
        f = self.lib.immesh_topology_manifold_new_vertices; f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]; f.restype = C.c_int
        n = C.c_int64(0)
        self._check(f(self.raycaster(), None, None, 0, C.byref(n)), "topology_manifold_new_vertices")
        vsrc, xyz = np.empty(n.value, np.int32), np.empty((n.value, 3), np.float32)
        self._check(f(self.raycaster(), _ptr(vsrc), _ptr(xyz), n.value, C.byref(n)), "topology_manifold_new_vertices")
        return vsrc, xyz

    def topology_manifold_apply(self):
        """immesh_topology_manifold_apply: vtx_out and faces_out become the caster's, on the device, and its hierarchy is built again; everything a
        build discards is discarded"""
        f = self.lib.immesh_topology_manifold_apply; f.argtypes = [C.c_void_p]; f.restype = C.c_int
        self._check(f(self.raycaster()), "topology_manifold_apply")

    def topology_manifold_timing(self):
        """device milliseconds of the last (manifold pass, apply)"""
        f = self.lib.immesh_topology_manifold_last_timing; f.argtypes = [C.c_void_p, C.c_void_p]; f.restype = C.c_int
        ms = (C.c_float * 2)()
        self._check(f(self.raycaster(), ms), "topology_manifold_last_timing")
        return float(ms[0]), float(ms[1])

    # -- weld and vertex clustering of the caster's snapshot (include/immesh_simplify.h) ---------------------------------------------------------------
    def simplify(self, cell=0.0, mode=SIMPLIFY_FIRST, merge_duplicates=True):
        """immesh_simplify on the caster's snapshot: cell == 0 welds the vertices of equal floats, cell > 0 clusters them on a grid (SIMPLIFY_FIRST:
        the label vertex stays, SIMPLIFY_MEAN: the members' mean); merge_duplicates drops faces over the same three new vertices -> SimplifyStats;
        the result stays on the device for the calls below"""
        f = self.lib.immesh_simplify; f.argtypes = [C.c_void_p, C.c_double, C.c_int32, C.c_int32, C.POINTER(SimplifyStats)]; f.restype = C.c_int
        st = SimplifyStats()
        self._check(f(self.raycaster(), cell, mode, 1 if merge_duplicates else 0, C.byref(st)), "simplify")
        return st

    def simplify_vertices(self):
        """the cluster tables -> dict: vtx (n_vertices_out, 3) float32, first_vertex, n_members (n_vertices_out,) int32"""
        f = self.lib.immesh_simplify_vertices; f.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p]; f.restype = C.c_int
        n = C.c_int64(0)
        self._check(f(self.raycaster(), None, None, None, 0, C.byref(n)), "simplify_vertices")
        out = {"vtx": np.empty((n.value, 3), np.float32), "first_vertex": np.empty(n.value, np.int32), "n_members": np.empty(n.value, np.int32)}
        self._check(f(self.raycaster(), *[_ptr(out[k]) for k in ("vtx", "first_vertex", "n_members")], n.value, C.byref(n)), "simplify_vertices")
        return out

    def simplify_maps(self):
        """-> dict: vmap (n_vtx,) int32 (-1: unused), fmap (n_faces,) int32 (-1: not kept), fstatus (n_faces,) int8"""
        f = self.lib.immesh_simplify_maps; f.argtypes = [C.c_void_p] + [C.c_void_p] * 3; f.restype = C.c_int
        self._check(f(self.raycaster(), None, None, None), "simplify_maps")
        nv, nf = self._raycast_sizes()[:2]
        out = {"vmap": np.empty(nv, np.int32), "fmap": np.empty(nf, np.int32), "fstatus": np.empty(nf, np.int8)}
        self._check(f(self.raycaster(), _ptr(out["vmap"]), _ptr(out["fmap"]), _ptr(out["fstatus"])), "simplify_maps")
        return out

    def simplify_faces(self):
        """the kept faces over the new vertex indices, in face order -> (n_faces_out, 3) int32"""
        f = self.lib.immesh_simplify_faces; f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]; f.restype = C.c_int
        n = C.c_int64(0)
        self._check(f(self.raycaster(), None, 0, C.byref(n)), "simplify_faces")
        out = np.empty((n.value, 3), np.int32)
        self._check(f(self.raycaster(), _ptr(out), n.value, C.byref(n)), "simplify_faces")
        return out

    def simplify_apply(self):
        """immesh_simplify_apply: vtx_out and faces_out become the caster's, on the device, and its hierarchy is built again; everything a build
        discards is discarded"""
        f = self.lib.immesh_simplify_apply; f.argtypes = [C.c_void_p]; f.restype = C.c_int
        self._check(f(self.raycaster()), "simplify_apply")

    def simplify_last_timing(self):
        """device milliseconds of the last (simplify pass, apply)"""
        f = self.lib.immesh_simplify_last_timing; f.argtypes = [C.c_void_p, C.c_void_p]; f.restype = C.c_int
        ms = (C.c_float * 2)()
        self._check(f(self.raycaster(), ms), "simplify_last_timing")
        return float(ms[0]), float(ms[1])

    # -- the one-ring table, Taubin smoothing and vertex normals of the caster's snapshot (include/immesh_smooth.h) -----------------------------------
    def smooth(self, n_steps=10, lam=0.5, mu=-0.53, border=SMOOTH_BORDER_FIXED):
        """immesh_smooth on the caster's snapshot: the one-ring table, the vertex classes and n_steps Jacobi steps with the factor lam on even and mu
        on odd steps (Taubin: mu < -lam < 0; Laplace: mu == lam); border says what a BORDER vertex averages over -> SmoothStats; the result stays on
        the device for the calls below"""
        f = self.lib.immesh_smooth; f.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_int32, C.POINTER(SmoothStats)]; f.restype = C.c_int
        st = SmoothStats()
        self._check(f(self.raycaster(), n_steps, lam, mu, border, C.byref(st)), "smooth")
        return st

    def smooth_vertices(self):
        """-> dict: vtx (n_vtx, 3) float32 (the positions after the last step), vclass (n_vtx,) int8"""
        f = self.lib.immesh_smooth_vertices; f.argtypes = [C.c_void_p] + [C.c_void_p] * 2; f.restype = C.c_int
        self._check(f(self.raycaster(), None, None), "smooth_vertices")
        nv = self._raycast_sizes()[0]
        out = {"vtx": np.empty((nv, 3), np.float32), "vclass": np.empty(nv, np.int8)}
        self._check(f(self.raycaster(), _ptr(out["vtx"]), _ptr(out["vclass"])), "smooth_vertices")
        return out

    def smooth_adjacency(self):
        """the one-ring table -> dict: row_start (n_vtx + 1,) int64, neighbours, uses (n_pairs,) int32"""
        f = self.lib.immesh_smooth_adjacency; f.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p]; f.restype = C.c_int
        n = C.c_int64(0)
        self._check(f(self.raycaster(), None, None, None, 0, C.byref(n)), "smooth_adjacency")
        nv = self._raycast_sizes()[0]
        out = {"row_start": np.empty(nv + 1, np.int64), "neighbours": np.empty(n.value, np.int32), "uses": np.empty(n.value, np.int32)}
        self._check(f(self.raycaster(), *[_ptr(out[k]) for k in ("row_start", "neighbours", "uses")], n.value, C.byref(n)), "smooth_adjacency")
        return out

    def smooth_apply(self):
        """immesh_smooth_apply: the smoothed positions become the caster's, on the device, and its hierarchy is built again; everything a build
        discards is discarded"""
        f = self.lib.immesh_smooth_apply; f.argtypes = [C.c_void_p]; f.restype = C.c_int
        self._check(f(self.raycaster()), "smooth_apply")

    def smooth_last_timing(self):
        """device milliseconds of the last (one-ring and classes, steps, apply)"""
        f = self.lib.immesh_smooth_last_timing; f.argtypes = [C.c_void_p, C.c_void_p]; f.restype = C.c_int
        ms = (C.c_float * 3)()
        self._check(f(self.raycaster(), ms), "smooth_last_timing")
        return float(ms[0]), float(ms[1]), float(ms[2])

    def vertex_normals(self, fetch=True):
        """immesh_vertex_normals of the caster's current snapshot -> (normals (n_vtx, 3) float32, or None without fetch; n_zero)"""
        f = self.lib.immesh_vertex_normals; f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]; f.restype = C.c_int
        out = np.empty((self._raycast_sizes()[0], 3), np.float32) if fetch else None
        n = C.c_int64(0)
        self._check(f(self.raycaster(), _ptr(out) if fetch else None, C.byref(n)), "vertex_normals")
        return out, n.value

    # -- self-intersections of the caster's snapshot (include/immesh_intersect.h) -----------------------------------------------------------------------
    def self_intersect(self, max_candidates=1 << 24):
        """immesh_self_intersect on the caster's snapshot: the candidate pairs (faces that take part, float boxes overlapping), their segment tests,
        the intersecting pairs and per face the number it is in -> IntersectStats; the result stays on the device for the calls below.  More than
        max_candidates candidates raise (rc=-4)"""
        f = self.lib.immesh_self_intersect; f.argtypes = [C.c_void_p, C.c_int64, C.POINTER(IntersectStats)]; f.restype = C.c_int
        st = IntersectStats()
        self._check(f(self.raycaster(), max_candidates, C.byref(st)), "self_intersect")
        return st

    def self_intersect_pairs(self):
        """the intersecting pairs in ascending (i, j) -> (pairs (n_pairs, 2) int32, mask (n_pairs,) uint8)"""
        f = self.lib.immesh_self_intersect_pairs; f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]; f.restype = C.c_int
        n = C.c_int64(0)
        self._check(f(self.raycaster(), None, None, 0, C.byref(n)), "self_intersect_pairs")
        pairs, mask = np.empty((n.value, 2), np.int32), np.empty(n.value, np.uint8)
        self._check(f(self.raycaster(), _ptr(pairs), _ptr(mask), n.value, C.byref(n)), "self_intersect_pairs")
        return pairs, mask

    def self_intersect_faces(self):
        """-> dict: n_partners (n_faces,) int32, face_map (n_faces,) int32 (the index after an apply, -1: the face goes)"""
        f = self.lib.immesh_self_intersect_faces; f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]; f.restype = C.c_int
        self._check(f(self.raycaster(), None, None), "self_intersect_faces")
        nf = self._raycast_sizes()[1]
        out = {"n_partners": np.empty(nf, np.int32), "face_map": np.empty(nf, np.int32)}
        self._check(f(self.raycaster(), _ptr(out["n_partners"]), _ptr(out["face_map"])), "self_intersect_faces")
        return out

    def self_intersect_apply(self):
        """immesh_self_intersect_apply: the faces without a partner become the caster's, on the device, and its hierarchy is built again; everything a
        build discards is discarded"""
        f = self.lib.immesh_self_intersect_apply; f.argtypes = [C.c_void_p]; f.restype = C.c_int
        self._check(f(self.raycaster()), "self_intersect_apply")

    def self_intersect_timing(self):
        """device milliseconds of the last (candidates, tests and sort, apply)"""
        f = self.lib.immesh_self_intersect_last_timing; f.argtypes = [C.c_void_p, C.c_void_p]; f.restype = C.c_int
        ms = (C.c_float * 3)()
        self._check(f(self.raycaster(), ms), "self_intersect_last_timing")
        return float(ms[0]), float(ms[1]), float(ms[2])

    # -- shaded and coloured images of the mesh (include/immesh_shade.h) -------------------------------------------------------------------------
    def default_shade(self, **over):
        return default_shade(self.lib, **over)

    def _shade_outputs(self, cam, want_rgb, want_depth, want_face):
        shape = (max(cam.height, 0), max(cam.width, 0))               # (a bad size is the library's to reject)
        return (np.empty(shape + (3,), np.uint8) if want_rgb else None, np.empty(shape, np.float32) if want_depth else None,
                np.empty(shape, np.int32) if want_face else None)

    def shade_triangles(self, cam, vtx_xyz, faces, shade, vtx_rgb=None, want_rgb=True, want_depth=True, want_face=True):
        """immesh_shade_triangles on a host triangle soup -> (rgb (h, w, 3) uint8, depth (h, w) float32, face (h, w) int32), None where not wanted"""
        f = self.lib.immesh_shade_triangles
        f.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(Shade), C.c_void_p, C.c_void_p,
                      C.c_void_p]
        f.restype = C.c_int
        vtx = np.ascontiguousarray(vtx_xyz, dtype=np.float32).reshape(-1, 3)
        fc = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
        col = None if vtx_rgb is None else np.ascontiguousarray(vtx_rgb, dtype=np.uint8).reshape(-1, 3)
        if col is not None and len(col) != len(vtx):
            raise ValueError("vtx_rgb must hold one byte triple per vertex")
        rgb, depth, face = self._shade_outputs(cam, want_rgb, want_depth, want_face)
        self._check(f(self.renderer(), C.byref(cam), _ptr(vtx), len(vtx), _ptr(fc), len(fc), _ptr(col), C.byref(shade), _ptr(rgb), _ptr(depth), _ptr(face)),
                    "shade_triangles")
        return rgb, depth, face

    def shade_mesh(self, cam, shade, smooth_factor=1.0, knn=20, colourer=True, want_rgb=True, want_depth=True, want_face=True):
        """immesh_shade_mesh: the live mesh as mesh_export(smooth_factor, knn) exports it -> (rgb, depth, face).  colourer: True = the context's own
        (created at first use) when the source is VERTEX, None / False = none, or a raw immesh_colourer pointer"""
        f = self.lib.immesh_shade_mesh
        f.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_void_p, C.c_double, C.c_int32, C.POINTER(Shade), C.c_void_p, C.c_void_p, C.c_void_p]
        f.restype = C.c_int
        if colourer is True:
            colourer = self.colourer() if shade.source == SHADE_VERTEX else None
        elif colourer is False:
            colourer = None
        rgb, depth, face = self._shade_outputs(cam, want_rgb, want_depth, want_face)
        self._check(f(self.renderer(), C.byref(cam), colourer, smooth_factor, knn, C.byref(shade), _ptr(rgb), _ptr(depth), _ptr(face)), "shade_mesh")
        return rgb, depth, face

    def shade_range(self):
        """the AXIS range (lo, hi) the last shade call used; (0, 0) when its source was not AXIS"""
        f = self.lib.immesh_shade_range; f.argtypes = [C.c_void_p, C.c_void_p]; f.restype = C.c_int
        lo_hi = (C.c_double * 2)()
        self._check(f(self.renderer(), lo_hi), "shade_range")
        return float(lo_hi[0]), float(lo_hi[1])

    def shade_timing(self):
        """device milliseconds of the last shade call's colour pass alone (render_timing has the same call's rasterize and reinforce)"""
        f = self.lib.immesh_renderer_last_shade_ms; f.argtypes = [C.c_void_p, C.c_void_p]; f.restype = C.c_int
        ms = C.c_float(0.0)
        self._check(f(self.renderer(), C.byref(ms)), "renderer_last_shade_ms")
        return float(ms.value)

    # -- vertex colours from camera images (include/immesh_colour.h) ----------------------------------------------------------------------------
    def colourer(self):
        """the context's colourer (created at first use, destroyed by close())"""
        if getattr(self, "_colourer", None) is None:
            f = self.lib.immesh_colourer_create; f.argtypes = [C.c_void_p]; f.restype = C.c_void_p
            r = f(self.ctx)
            if not r:
                self._check(-1, "colourer_create")
            self._colourer = C.c_void_p(r)
        return self._colourer

    def default_image(self, pixels=None, **over):
        return default_image(self.lib, pixels, **over)

    def colour_image(self, im, model=COLOUR_PLAIN, set=COLOUR_SET_ALL, ids=None, select_min_dis=0.0):
        """immesh_colour_image: one camera frame onto the vertex colours -> the call's statistics as a dict"""
        f = self.lib.immesh_colour_image
        f.argtypes = [C.c_void_p, C.POINTER(Image), C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_double, C.POINTER(ColourStats)]; f.restype = C.c_int
        ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
        st = ColourStats()
        self._check(f(self.colourer(), C.byref(im), model, set, _ptr(ids), 0 if ids is None else len(ids), select_min_dis, C.byref(st)), "colour_image")
        return {n: getattr(st, n) for n, _ in ColourStats._fields_}

    def colour_selected(self):
        """the render set of the last colour_image -> (ids (n,) int32 ascending, raw uv (n, 2) float32)"""
        f = self.lib.immesh_colour_selected; f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]; f.restype = C.c_int
        n = C.c_int64(0)
        self._check(f(self.colourer(), None, None, 0, C.byref(n)), "colour_selected")
        ids, uv = np.zeros(n.value, np.int32), np.zeros((n.value, 2), np.float32)
        self._check(f(self.colourer(), _ptr(ids), _ptr(uv), n.value, C.byref(n)), "colour_selected")
        return ids, uv

    def colour_fetch(self, ids=None, n=None):
        """immesh_colour_fetch: ids, or (None) the first n vertices (default: every vertex of the map) -> (rgb (n, 3) uint8, states COLOUR_STATE_DTYPE)"""
        f = self.lib.immesh_colour_fetch; f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]; f.restype = C.c_int
        if ids is not None:
            ids = np.ascontiguousarray(ids, dtype=np.int32); n = len(ids)
        elif n is None:
            n = self.counters()["n_vertices"]
        rgb, st = np.zeros((n, 3), np.uint8), np.zeros(n, COLOUR_STATE_DTYPE)
        self._check(f(self.colourer(), _ptr(ids), n, _ptr(rgb), _ptr(st)), "colour_fetch")
        return rgb, st

    def save_ply_rgb(self, path, smooth_factor=1.0, knn=20, min_views=0, bgr=True):
        f = self.lib.immesh_save_ply_rgb; f.argtypes = [C.c_void_p, C.c_char_p, C.c_double, C.c_int32, C.c_int32, C.c_int32]; f.restype = C.c_int
        self._check(f(self.colourer(), path.encode(), smooth_factor, knn, min_views, 1 if bgr else 0), "save_ply_rgb")

    def colour_timing(self):
        """device milliseconds of the last colour_image: (upload, select, update)"""
        f = self.lib.immesh_colourer_last_timing; f.argtypes = [C.c_void_p, C.c_void_p]; f.restype = C.c_int
        ms = (C.c_float * 3)()
        self._check(f(self.colourer(), ms), "colourer_last_timing")
        return float(ms[0]), float(ms[1]), float(ms[2])

    # -- checkpoints (include/immesh_checkpoint.h) -------------------------------------------------------------------------------------------------
    def _checkpoint(self, which, path, colourer):
        f = getattr(self.lib, "immesh_checkpoint_" + which)
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.POINTER(CheckpointInfo)]; f.restype = C.c_int
        col = self.colourer() if colourer is True else (getattr(self, "_colourer", None) if colourer is None else (colourer or None))
        info = CheckpointInfo()
        rc = f(self.ctx, col, os.fsencode(path), C.byref(info))
        if rc != 0:
            g = self.lib.immesh_last_error; g.restype = C.c_char_p; g.argtypes = [C.c_void_p]
            raise CheckpointError("immesh_checkpoint_" + which, rc, g(self.ctx).decode())
        return _checkpoint_info_dict(info)

    def checkpoint_save(self, path, colourer=None):
        """immesh_checkpoint_save -> info dict.  colourer: None = the context's colourer if one was created, True = create one, False = without colours"""
        return self._checkpoint("save", path, colourer)

    def checkpoint_load(self, path, colourer=None):
        """immesh_checkpoint_load into this (unused) context -> info dict; colourer as for checkpoint_save"""
        return self._checkpoint("load", path, colourer)

    def checkpoint_probe(self, path):
        return checkpoint_probe(self.lib, path)

    def process_scan_strided(self, down_bytes, n_ds, down_stride, raw_bytes, n_raw, raw_stride, raw_int_off, state_prior, state, frame_idx=0, do_mesh=True):
        """immesh_process_scan_strided: down_bytes / raw_bytes = numpy arrays (any dtype) or device pointers holding the pcl-shaped clouds"""
        f = self._f("process_scan_strided"); f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        out = np.array(state, dtype=np.float64, copy=True)
        n_iter, n_match = C.c_int32(0), C.c_int32(0)
        self._check(f(self.ctx, _ptr(down_bytes), n_ds, down_stride, _ptr(raw_bytes), n_raw, raw_stride, raw_int_off, _ptr(np.ascontiguousarray(state_prior, dtype=np.float64)),
                      _ptr(out), frame_idx, int(do_mesh), C.byref(n_iter), C.byref(n_match)), "process_scan_strided")
        return out, {"n_iter": n_iter.value, "n_match": n_match.value}

    # -- whole scan -------------------------------------------------------------------------------------------
    def process_scan(self, pts_down, pts_raw_xyzi, state_prior, state, frame_idx=0, do_mesh=True, n_ds=None, n_raw=None):
        f = self._f("process_scan"); f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        n_ds = len(pts_down) if n_ds is None else n_ds
        n_raw = len(pts_raw_xyzi) if n_raw is None else n_raw
        out = np.array(state, dtype=np.float64, copy=True)
        n_iter, n_match = C.c_int32(0), C.c_int32(0)
        self._check(f(self.ctx, _ptr(pts_down), n_ds, _ptr(pts_raw_xyzi), n_raw, _ptr(np.ascontiguousarray(state_prior, dtype=np.float64)),
                      _ptr(out), frame_idx, int(do_mesh), C.byref(n_iter), C.byref(n_match)), "process_scan")
        return out, {"n_iter": n_iter.value, "n_match": n_match.value}

    def last_timing(self):
        f = self._f("last_timing"); f.argtypes = [C.c_void_p, C.c_void_p]; f.restype = C.c_int
        ms = np.zeros(4, np.float32)
        self._check(f(self.ctx, _ptr(ms)), "last_timing")
        return {"total": float(ms[0]), "register": float(ms[1]), "map_update": float(ms[2]), "mesh": float(ms[3])}

    # -- the stage before the path: VoxelGrid down-sampling ----------------------------------------------------
    def downsample(self, pts, leaf, n=None, stride=None, to_host=True):
        """pts: host ndarray (n x 3 or n x 4 float32) or device pointer (then pass n and stride).  Returns (host array | None, n_out)."""
        f = self._f("downsample"); f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_int32, C.c_void_p]
        if n is None:
            n, stride = pts.shape[0], pts.shape[1]
        out = np.zeros((n, 3), np.float32) if to_host else None
        n_out = C.c_int32(0)
        self._check(f(self.ctx, _ptr(pts), n, stride, leaf, _ptr(out), n, C.byref(n_out)), "downsample")
        return (out[:n_out.value] if to_host else None), n_out.value

    def decode_livox(self, wire_points, n_scans=6, point_filter_num=1, blind=1.0, to_host=True):
        """avia_handler: wire_points = n x 19 uint8 (serialised livox CustomPoint).  Returns (n_out x 5 float32 | None, n_out)."""
        f = self._f("decode_livox"); f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p]
        w = np.ascontiguousarray(wire_points, dtype=np.uint8).reshape(-1, 19)
        out = np.zeros((len(w), 5), np.float32) if to_host else None
        n_out = C.c_int32(0)
        self._check(f(self.ctx, _ptr(w), len(w), n_scans, point_filter_num, blind, _ptr(out), C.byref(n_out)), "decode_livox")
        return (out[:n_out.value] if to_host else None), n_out.value

    def decode_velodyne(self, data, point_step, offsets, n_scans=64, to_host=True):
        """velodyne_handler: data = n x point_step uint8 (PointCloud2.data); offsets = byte offsets of x, y, z, intensity."""
        f = self._f("decode_velodyne"); f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int32] * 7 + [C.c_void_p, C.c_void_p]
        d = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1, point_step)
        out = np.zeros((len(d), 5), np.float32) if to_host else None
        n_out = C.c_int32(0)
        self._check(f(self.ctx, _ptr(d), len(d), point_step, offsets[0], offsets[1], offsets[2], offsets[3], n_scans, _ptr(out), C.byref(n_out)), "decode_velodyne")
        return (out[:n_out.value] if to_host else None), n_out.value

    def decode_result_ptr(self):
        f = self._f("decode_result"); f.argtypes = [C.c_void_p]; f.restype = C.c_void_p
        return f(self.ctx)

    def undistort(self, pts_xyzit, imu, lidar_beg_time, last_update_time, imu_ctx, state, to_host=True):
        """UndistortPcl.  pts_xyzit: n x 5 float32 (x y z intensity offset_ms); imu: m x 7 float64 (t, gyr, acc).
        Returns (cloud n x 4 in time order | None, propagated state, last_update_time); imu_ctx is updated in place."""
        f = self._f("undistort"); f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        imu = np.ascontiguousarray(imu, dtype=np.float64).reshape(-1, 7)
        out = np.zeros((len(pts_xyzit), 4), np.float32) if to_host else None
        st = np.array(state, dtype=np.float64, copy=True)
        lut = C.c_double(last_update_time)
        self._check(f(self.ctx, _ptr(np.ascontiguousarray(pts_xyzit, dtype=np.float32)), len(pts_xyzit), _ptr(imu), len(imu), lidar_beg_time,
                      C.byref(lut), C.byref(imu_ctx), _ptr(st), _ptr(out)), "undistort")
        return out, st, lut.value

    def undistort_result_ptr(self):
        f = self._f("undistort_result"); f.argtypes = [C.c_void_p]; f.restype = C.c_void_p
        return f(self.ctx)

    # -- legacy registration path ------------------------------------------------------------
    def ikd_build(self, pts_world_xyz, downsample_size):
        f = self._f("ikd_build"); f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_double]; f.restype = C.c_int
        p = np.ascontiguousarray(pts_world_xyz, dtype=np.float32)
        self._check(f(self.ctx, _ptr(p), len(p), downsample_size), "ikd_build")

    def ikd_add_points(self, pts_world_xyz):
        f = self._f("ikd_add_points"); f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]; f.restype = C.c_int
        p = np.ascontiguousarray(pts_world_xyz, dtype=np.float32)
        self._check(f(self.ctx, _ptr(p), len(p)), "ikd_add_points")

    def ikd_delete_boxes(self, boxes):
        f = self._f("ikd_delete_boxes"); f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]; f.restype = C.c_int
        b = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 6)
        n = C.c_int32(0)
        self._check(f(self.ctx, _ptr(b), len(b), C.byref(n)), "ikd_delete_boxes")
        return n.value

    def ikd_fov_segment(self, pos_lid, cube_len, detection_range):
        f = self._f("ikd_fov_segment"); f.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p]; f.restype = C.c_int
        n = C.c_int32(0)
        self._check(f(self.ctx, _ptr(np.ascontiguousarray(pos_lid, dtype=np.float64)), cube_len, detection_range, C.byref(n)), "ikd_fov_segment")
        return n.value

    def ikd_size(self):
        f = self._f("ikd_size"); f.argtypes = [C.c_void_p, C.c_void_p]; f.restype = C.c_int
        n = C.c_int64(0)
        self._check(f(self.ctx, C.byref(n)), "ikd_size")
        return n.value

    def ikd_dump(self):
        """all map points, sorted lexicographically by (x, y, z)"""
        f = self._f("ikd_dump"); f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]; f.restype = C.c_int
        cap = self.ikd_size()
        out = np.zeros((max(cap, 1), 3), np.float32)
        n = C.c_int64(0)
        self._check(f(self.ctx, _ptr(out), cap, C.byref(n)), "ikd_dump")
        out = out[:min(cap, n.value)]
        return out[np.lexsort((out[:, 2], out[:, 1], out[:, 0]))]

    def ikd_knn(self, q_xyz):
        f = self._f("ikd_knn"); f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]; f.restype = C.c_int
        q = np.ascontiguousarray(q_xyz, dtype=np.float32)
        nn = np.zeros((len(q), 5, 3), np.float32); d2 = np.zeros((len(q), 5), np.float32); nf = np.zeros(len(q), np.int32)
        self._check(f(self.ctx, _ptr(q), len(q), _ptr(nn), _ptr(d2), _ptr(nf)), "ikd_knn")
        return nn, d2, nf

    def ikd_register(self, pts_down_body, state_prior, state, laser_point_cov=0.001):
        f = self._f("ikd_register"); f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        p = np.ascontiguousarray(pts_down_body, dtype=np.float32)
        n = len(p)
        out = np.array(state, dtype=np.float64, copy=True)
        n_iter, n_match, res = C.c_int32(0), C.c_int32(0), C.c_double(0)
        idx = np.zeros(n, np.int32); nv = np.zeros((n, 4), np.float32)
        self._check(f(self.ctx, _ptr(p), n, _ptr(np.ascontiguousarray(state_prior, dtype=np.float64)), _ptr(out), laser_point_cov, C.byref(n_iter),
                      C.byref(n_match), C.byref(res), _ptr(idx), _ptr(nv)), "ikd_register")
        m = n_match.value
        return out, {"n_iter": n_iter.value, "n_match": m, "res_mean": res.value, "match_idx": idx[:m].copy(), "normals_pd2": nv[:m].copy()}

    def downsample_begin(self, pts, leaf, n=None, stride=None):
        """enqueue the VoxelGrid of a (host array | device pointer) cloud on the pre-processing stream; collect with downsample_end()"""
        f = self._f("downsample_begin"); f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double]; f.restype = C.c_int
        if n is None:
            n, stride = pts.shape[0], pts.shape[1]
        self._ds_keep = pts       # (a host array has to outlive the staging copy)
        self._check(f(self.ctx, _ptr(pts), n, stride, leaf), "downsample_begin")

    def downsample_end(self):
        """-> (n_out, pointer of the n_out x 3 float32 result: device memory for the HIP library, host memory for the oracle)"""
        f = self._f("downsample_end"); f.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_void_p)]; f.restype = C.c_int
        n = C.c_int32(0); ptr = C.c_void_p(0)
        self._check(f(self.ctx, C.byref(n), C.byref(ptr)), "downsample_end")
        return n.value, ptr.value

    def inputs_consumed(self):
        """block until the last asynchronous process_scan has consumed its (device-resident) input clouds"""
        f = self._f("inputs_consumed"); f.argtypes = [C.c_void_p]; f.restype = C.c_int
        self._check(f(self.ctx), "inputs_consumed")

    def last_matches(self):
        """(matched body points n x 3, normal + residual n x 4) of the last registration on the context"""
        f = self._f("last_matches"); f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]; f.restype = C.c_int
        n = C.c_int32(0)
        self._check(f(self.ctx, None, None, 0, C.byref(n)), "last_matches")
        p, q = np.zeros((n.value, 3), np.float32), np.zeros((n.value, 4), np.float32)
        if n.value:
            self._check(f(self.ctx, _ptr(p), _ptr(q), n.value, C.byref(n)), "last_matches")
        return p, q

    def mesh_collect_enable(self, on=True):
        f = self._f("mesh_collect_enable"); f.argtypes = [C.c_void_p, C.c_int32]; f.restype = C.c_int
        self._check(f(self.ctx, 1 if on else 0), "mesh_collect_enable")

    def mesh_collect_begin(self, timeout_ms=1000):
        """-> job ordinal, or None when no job finished within the timeout"""
        f = self._f("mesh_collect_begin"); f.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]; f.restype = C.c_int
        o = C.c_int64(0)
        rc = f(self.ctx, timeout_ms, C.byref(o))
        if rc == 1:
            return None
        self._check(rc, "mesh_collect_begin")
        return o.value

    def mesh_collect_end(self):
        f = self._f("mesh_collect_end"); f.argtypes = [C.c_void_p]; f.restype = C.c_int
        self._check(f(self.ctx), "mesh_collect_end")

    def registration_fallbacks(self):
        f = self._f("registration_fallbacks"); f.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]; f.restype = C.c_int
        n = C.c_int64(0)
        self._check(f(self.ctx, C.byref(n)), "registration_fallbacks")
        return n.value

    def downsample_result_ptr(self):
        f = self._f("downsample_result"); f.argtypes = [C.c_void_p]; f.restype = C.c_void_p
        return f(self.ctx)

    # -- multi-GPU sharding ------------------------------------------------------------------------------------
    def set_allreduce(self, fn):
        """fn(np.ndarray float64 view of the library's buffer) must sum it over all ranks IN PLACE (e.g. torch.distributed.all_reduce)."""
        proto = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.c_int32, C.c_void_p)

        def _cb(buf, n, user):
            try:
                fn(np.ctypeslib.as_array(buf, shape=(n,)))
                return 0
            except Exception:   # never raise through the C frame
                return -1
        self._allreduce_cb = proto(_cb)   # keep alive
        f = self._f("set_allreduce"); f.argtypes = [C.c_void_p, proto, C.c_void_p]; f.restype = C.c_int
        self._check(f(self.ctx, self._allreduce_cb, None), "set_allreduce")

    def stub_collectives(self):
        f = self._f("stub_collectives"); f.argtypes = [C.c_void_p]; f.restype = C.c_int
        self._check(f(self.ctx), "stub_collectives")

    def device_bytes(self):
        f = self._f("device_bytes"); f.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]; f.restype = C.c_int
        b = C.c_int64(0)
        self._check(f(self.ctx, C.byref(b)), "device_bytes")
        return b.value

    # -- RCCL inside the library (sharded contexts) ----------------------------------------------------------------
    def rccl_unique_id(self):
        f = self._f("rccl_unique_id"); f.argtypes = [C.c_void_p]; f.restype = C.c_int
        uid = np.zeros(128, np.uint8)
        rc = f(_ptr(uid))
        if rc != 0:
            e = self._f("rccl_error"); e.restype = C.c_char_p
            raise RuntimeError(f"immesh_rccl_unique_id failed rc={rc}: {e().decode()}")
        return uid

    def rccl_init(self, uid):
        f = self._f("rccl_init"); f.argtypes = [C.c_void_p, C.c_void_p]; f.restype = C.c_int
        self._check(f(self.ctx, _ptr(np.ascontiguousarray(uid, np.uint8))), "rccl_init")

    def set_threads(self, mesher_threads, matcher_threads):
        """oracle only (CPU baseline leg): the reference's own threading -- a 12-thread pool over mesh voxels, 4 OpenMP threads in the matcher"""
        f = self._f("set_threads"); f.argtypes = [C.c_void_p, C.c_int32, C.c_int32]; f.restype = C.c_int
        self._check(f(self.ctx, mesher_threads, matcher_threads), "set_threads")

    def set_allgather(self, fn):
        """Sharded mesher.  fn(send: uint8 view [nbytes], recv: uint8 view [world * nbytes]) gathers every rank's `send` into `recv` in
        rank order (e.g. torch.distributed.all_gather_into_tensor)."""
        proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p)
        world = max(1, int(self.cfg.shard_world))

        def _cb(send, nbytes, recv, user):
            try:
                s = np.ctypeslib.as_array(C.cast(send, C.POINTER(C.c_uint8)), shape=(nbytes,))
                r = np.ctypeslib.as_array(C.cast(recv, C.POINTER(C.c_uint8)), shape=(nbytes * world,))
                fn(s, r)
                return 0
            except Exception:   # never raise through the C frame
                import traceback
                traceback.print_exc()
                return -1
        self._allgather_cb = proto(_cb)   # keep alive
        f = self._f("set_allgather"); f.argtypes = [C.c_void_p, proto, C.c_void_p]; f.restype = C.c_int
        self._check(f(self.ctx, self._allgather_cb, None), "set_allgather")

    def broadcast_scan(self, pts, root=0, stride=None, n=None):
        """immesh_broadcast_scan: collective; the root passes the scan (ndarray n x 3 / n x 4 or a device pointer with n and stride), the others None.
        Returns (device pointer, points) of the scan in this context's memory."""
        f = self._f("broadcast_scan"); f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        if pts is not None and not isinstance(pts, (int, np.integer)):
            pts = np.ascontiguousarray(pts, np.float32)
            n, stride = len(pts), pts.shape[1]
        out, n_out = C.c_void_p(0), C.c_int32(0)
        self._check(f(self.ctx, _ptr(pts), int(n or 0), int(stride or 0), int(root), C.byref(out), C.byref(n_out)), "broadcast_scan")
        return int(out.value), int(n_out.value)

    def shard_traffic(self):
        f = self._f("shard_traffic"); f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]; f.restype = C.c_int
        b, n = C.c_int64(0), C.c_int64(0)
        self._check(f(self.ctx, C.byref(b), C.byref(n)), "shard_traffic")
        return {"bytes": b.value, "calls": n.value}

    # -- per-kernel timing (product library only) --------------------------------------------------------------
    def profile_enable(self, on=True):
        f = self._f("profile_enable"); f.argtypes = [C.c_void_p, C.c_int32]; f.restype = C.c_int
        self._check(f(self.ctx, 1 if on else 0), "profile_enable")

    def profile_read(self, reset=False):
        f = self._f("profile_read"); f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]; f.restype = C.c_int
        buf = (KernelStat * 128)()
        n = C.c_int32(0)
        self._check(f(self.ctx, C.byref(buf), 128, C.byref(n), 1 if reset else 0), "profile_read")
        return {buf[i].name.decode(): {"launches": buf[i].launches, "total_ms": buf[i].total_ms} for i in range(min(n.value, 128))}

    # -- introspection ----------------------------------------------------------------------------------------
    def dump_planes(self, cap=None):
        """all initialised octree nodes (unordered); cap = at most that many records (a sample of a big map)"""
        f = self._f("dump_planes"); f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]; f.restype = C.c_int
        n = C.c_int64(0)
        self._check(f(self.ctx, None, 0, C.byref(n)), "dump_planes")
        m = n.value if cap is None else min(n.value, int(cap))
        recs = np.zeros(m, PLANE_DTYPE)
        if m:
            self._check(f(self.ctx, _ptr(recs), m, C.byref(n)), "dump_planes")
        return recs

    def counters(self, reset=False):
        f = self._f("counters"); f.argtypes = [C.c_void_p, C.POINTER(Counters), C.c_int32]; f.restype = C.c_int
        c = Counters()
        self._check(f(self.ctx, C.byref(c), 1 if reset else 0), "counters")
        return {n: getattr(c, n) for n in COUNTER_FIELDS}
