"""ctypes binding of libnr.so (C ABI: include/neural_render.h).

The shared library is built in-tree (``make -C cudaneuralrender_amd/csrc``, or
``__graft_entry__.build()``) into ``cudaneuralrender_amd/lib/libnr.so``.  There is
no fallback: if the library is missing, importing the compute API raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# NR_LIBRARY: an alternative build of the same ABI (A/B experiments under tools/)
LIB_PATH = os.environ.get("NR_LIBRARY") or os.path.join(_HERE, "lib", "libnr.so")

NR_OK = 0
NR_PRECISION = {"fp32": 0, "bf16": 1, "fp16": 2, "fp32x3": 3}
NR_SCENE = {"v1": 0, "tanh": 1, "subtract": 2, "cylinders": 3, "displace": 4, "round": 5}
NR_COLOR_FACING, NR_COLOR_MATCAP = 0, 1
NR_HOST, NR_DEVICE = 0, 1
NR_SCHEDULE = {"persistent": 0, "wavefront": 1, "layered": 2}
NR_GROUP_COPY, NR_GROUP_ASYNC = 1, 2
NR_ENDGAME_DEFAULT = 0.001  # include/neural_render.h: the bf16/fp16 endgame threshold by default
# status of a queried ray (nr_trace_rays, nr_render_gbuffer)
NR_RAY_MISS, NR_RAY_ESCAPED, NR_RAY_HIT, NR_RAY_LIMIT = 0, 1, 2, 3
# nr_render_aa: which pixels are resolved from their S x S samples, and the default edge contrast
NR_AA_MODE = {"adaptive": 0, "full": 1}
NR_AA_CONTRAST_DEFAULT = 32
# status of a projected point (nr_project_points)
NR_PROJ_CONVERGED, NR_PROJ_LIMIT, NR_PROJ_FLAT = 0, 1, 2

# every symbol include/neural_render.h declares
EXPORTS = [
    "nr_create", "nr_destroy", "nr_last_error", "nr_abi_version", "nr_set_stream", "nr_synchronize",
    "nr_load_h5", "nr_load_mlp", "nr_mlp_info", "nr_set_precision", "nr_set_view", "nr_set_static",
    "nr_set_scene", "nr_set_matcap", "nr_render", "nr_render_shard", "nr_render_batch", "nr_shard_rows",
    "nr_assemble_shards", "nr_mlp_forward", "nr_layer_forward", "nr_camera", "nr_camera_ex", "nr_h5_read_keras",
    "nr_png_load", "nr_png_save", "nr_ppm_save", "nr_free", "nr_set_profiling", "nr_prof_collect",
    "nr_set_poll_interval", "nr_set_schedule", "nr_set_debug", "nr_debug_stamps",
    "nr_set_occupancy", "nr_set_temporal_order", "nr_dense_forward", "nr_set_pixel_spread", "nr_set_cost_probe", "nr_set_wave_rays", "nr_set_queue_shards", "nr_set_layer_chunk", "nr_batch_frames_per_launch",
    "nr_h5_open", "nr_h5_close", "nr_h5_root", "nr_h5_object_type", "nr_h5_num_members", "nr_h5_member",
    "nr_h5_dims", "nr_h5_read_f32",
    "nr_group_create", "nr_group_destroy", "nr_group_size", "nr_group_render_batch", "nr_pack_x3",
    "nr_set_endgame", "nr_group_create_ex", "nr_group_synchronize", "nr_group_layout",
    "nr_trace_rays", "nr_render_gbuffer", "nr_render_aa", "nr_render_lit",
    "nr_sample_grid", "nr_mesh_grid", "nr_extract_mesh", "nr_extract_mesh_sparse", "nr_obj_save",
    "nr_mlp_gradient", "nr_project_points",
    "nr_pack_fp32_pruned", "nr_set_prune", "nr_prune_info", "nr_prune_redos",
    "nr_set_unit_skip", "nr_unit_skip_counts", "nr_pack_fp32_units",
    "nr_compose_create", "nr_compose_destroy", "nr_compose_bound", "nr_compose_set_parts", "nr_compose_info",
    "nr_compose_sample", "nr_compose_trace_rays", "nr_compose_gbuffer", "nr_compose_render",
    "nr_compose_sample_grid", "nr_compose_extract_mesh", "nr_compose_extract_mesh_sparse",
    "nr_compose_render_lit",
    "nr_fit_create", "nr_fit_destroy", "nr_fit_num_params", "nr_fit_gradient", "nr_fit_run", "nr_fit_weights",
    "nr_obj_load", "nr_trimesh_normals", "nr_trimesh_create", "nr_trimesh_destroy", "nr_trimesh_info",
    "nr_trimesh_distance", "nr_mesh_hierarchy", "nr_mesh_winding",
    "nr_mesh_trace_rays", "nr_mesh_gbuffer", "nr_mesh_render",
    "nr_mesh_area_table", "nr_mesh_sample", "nr_points_order", "nr_mesh_fit_samples",
    "nr_mesh_sample_grid", "nr_mesh_remesh", "nr_mesh_remesh_sparse",
    "nr_mesh_create_device", "nr_mesh_download",
]
# nr_trimesh_distance: flags, and the feature codes of its `feature` output
NR_TRIMESH_BRUTE = 1
# nr_mesh_trace_rays / nr_mesh_gbuffer / nr_mesh_render: further flags
NR_MESH_RAY_ANY, NR_MESH_RAY_SMOOTH = 2, 4
# nr_mesh_fit_samples: where the sign of Y comes from; nr_points_order: the key
NR_SAMPLE_SIGN = {"normal": 0, "winding": 1}
NR_ORDER = {"morton": 0, "shuffle": 1}
NR_TRIMESH_FEATURE = ("face", "edge AB", "edge BC", "edge CA", "vertex A", "vertex B", "vertex C")
# composed scenes (nr_compose_*): limits and part ops
NR_COMPOSE_MAX_NETS, NR_COMPOSE_MAX_PARTS = 4, 16
NR_PART_OP = {"union": 0, "subtract": 1}


class NRStats(ctypes.Structure):
    _fields_ = [
        ("ray_steps", ctypes.c_uint64),
        ("shade_evals", ctypes.c_uint64),
        ("rays_hit", ctypes.c_uint64),
        ("rays_shaded", ctypes.c_uint64),
        ("iterations", ctypes.c_int32),
        ("launches", ctypes.c_int32),
        ("ms_total", ctypes.c_float),
        ("endgame_evals", ctypes.c_uint64),
        ("endgame_switches", ctypes.c_uint64),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class NRFrame(ctypes.Structure):
    """nr_frame: one frame of nr_render_batch."""
    _fields_ = [
        ("inv_view", ctypes.c_float * 12),
        ("normal", ctypes.c_float * 16),
        ("frame", ctypes.c_int),
        ("out", ctypes.c_void_p),
    ]


class NRLight(ctypes.Structure):
    """nr_light: the directional light of nr_render_lit."""
    _fields_ = [
        ("dir", ctypes.c_float * 3),
        ("shadow_steps", ctypes.c_int),
        ("shadow_bias", ctypes.c_float),
        ("shadow_k", ctypes.c_float),
        ("ao_step", ctypes.c_float),
        ("ao_strength", ctypes.c_float),
        ("ambient", ctypes.c_float),
    ]


class NRProjectOpts(ctypes.Structure):
    """nr_project_opts: the level set, tolerance and step limits of nr_project_points."""
    _fields_ = [
        ("iso", ctypes.c_float),
        ("tol", ctypes.c_float),
        ("max_step", ctypes.c_float),
        ("max_iters", ctypes.c_int),
    ]


class NRFitOpts(ctypes.Structure):
    """nr_fit_opts: Adam's constants, the residual clamp, the partial sums and the grid of nr_fit_*."""
    _fields_ = [
        ("lr", ctypes.c_float),
        ("beta1", ctypes.c_float),
        ("beta2", ctypes.c_float),
        ("eps", ctypes.c_float),
        ("clamp", ctypes.c_float),
        ("partials", ctypes.c_int),
        ("grid", ctypes.c_int),
    ]


class NRSampleOpts(ctypes.Structure):
    """nr_sample_opts: the seed, counts, jitter, box and sign of nr_mesh_sample / nr_mesh_fit_samples."""
    _fields_ = [
        ("seed", ctypes.c_uint64),
        ("n_surface", ctypes.c_long),
        ("n_volume", ctypes.c_long),
        ("sigma", ctypes.c_float),
        ("lo", ctypes.c_float * 3),
        ("hi", ctypes.c_float * 3),
        ("sign", ctypes.c_int),
        ("beta", ctypes.c_float),
    ]


class NRPart(ctypes.Structure):
    """nr_part: one placed network of a composition."""
    _fields_ = [
        ("net", ctypes.c_int),
        ("op", ctypes.c_int),
        ("rot", ctypes.c_float * 9),
        ("pos", ctypes.c_float * 3),
        ("scale", ctypes.c_float),
    ]


class NRComposeStats(ctypes.Structure):
    _fields_ = [
        ("ray_steps", ctypes.c_uint64),
        ("shade_evals", ctypes.c_uint64),
        ("rays_hit", ctypes.c_uint64),
        ("rays_shaded", ctypes.c_uint64),
        ("part_evals", ctypes.c_uint64),
        ("wave_evals", ctypes.c_uint64),
        ("wave_skips", ctypes.c_uint64),
        ("iterations", ctypes.c_int32),
        ("launches", ctypes.c_int32),
        ("ms_total", ctypes.c_float),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class NRKernelProf(ctypes.Structure):
    _fields_ = [
        ("march_ms", ctypes.c_double),
        ("shade_ms", ctypes.c_double),
        ("init_ms", ctypes.c_double),
        ("march_launches", ctypes.c_uint64),
        ("shade_launches", ctypes.c_uint64),
        ("init_launches", ctypes.c_uint64),
        ("renders", ctypes.c_uint64),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class NRError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[nr error {code}] {msg}")
        self.code = code


_lib = None


def lib():
    """Load libnr.so (once).  Raises if the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"libnr.so not built: {LIB_PATH} missing (run __graft_entry__.build())")
    L = ctypes.CDLL(LIB_PATH)
    P, I, F, L64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_long
    FP = ctypes.POINTER(ctypes.c_float)
    IP = ctypes.POINTER(ctypes.c_int)
    sig = {
        "nr_create": (I, [I, ctypes.POINTER(P)]),
        "nr_destroy": (I, [P]),
        "nr_last_error": (ctypes.c_char_p, [P]),
        "nr_abi_version": (I, []),
        "nr_set_stream": (I, [P, P, I]),
        "nr_synchronize": (I, [P]),
        "nr_load_h5": (I, [P, ctypes.c_char_p]),
        "nr_load_mlp": (I, [P, I, IP, ctypes.POINTER(FP), ctypes.POINTER(FP)]),
        "nr_pack_x3": (I, [I, IP, ctypes.POINTER(FP), ctypes.POINTER(FP), P, ctypes.c_long, P, ctypes.c_long,
                           ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_long), IP]),
        "nr_mlp_info": (I, [P, IP, IP, IP, IP]),
        "nr_set_precision": (I, [P, I]),
        "nr_set_view": (I, [P, FP, FP, I]),
        "nr_set_static": (I, [P, I, I]),
        "nr_set_scene": (I, [P, I]),
        "nr_set_matcap": (I, [P, P, I, I]),
        "nr_render": (I, [P, P, I, I, I, I, ctypes.POINTER(NRStats)]),
        "nr_trace_rays": (I, [P, P, P, L64, I, P, P, P, P, P, I, ctypes.POINTER(NRStats)]),
        "nr_render_gbuffer": (I, [P, I, I, I, P, P, P, P, P, I, ctypes.POINTER(NRStats)]),
        "nr_render_aa": (I, [P, P, I, I, I, I, I, I, I, ctypes.POINTER(L64), ctypes.POINTER(NRStats)]),
        "nr_render_lit": (I, [P, P, I, I, I, ctypes.POINTER(NRLight), P, P, I, ctypes.POINTER(NRStats)]),
        "nr_sample_grid": (I, [P, FP, FP, IP, P, I, ctypes.POINTER(NRStats)]),
        "nr_mesh_grid": (I, [P, P, FP, FP, IP, F, P, L64, P, L64, ctypes.POINTER(L64), ctypes.POINTER(L64), I]),
        "nr_extract_mesh": (I, [P, FP, FP, IP, F, P, P, L64, P, L64, ctypes.POINTER(L64), ctypes.POINTER(L64), I,
                                ctypes.POINTER(NRStats)]),
        "nr_extract_mesh_sparse": (I, [P, FP, FP, IP, F, I, F, P, P, P, L64, P, L64, ctypes.POINTER(L64), ctypes.POINTER(L64),
                                       ctypes.POINTER(L64), I, ctypes.POINTER(NRStats)]),
        "nr_obj_save": (I, [ctypes.c_char_p, P, L64, P, P, L64]),
        "nr_render_shard": (I, [P, P, I, I, I, I, I, I, I, ctypes.POINTER(NRStats)]),
        "nr_render_batch": (I, [P, ctypes.POINTER(NRFrame), I, I, I, I, I, I, I, I, ctypes.POINTER(NRStats)]),
        "nr_group_create": (I, [ctypes.POINTER(P), I, ctypes.POINTER(P)]),
        "nr_group_destroy": (I, [P]),
        "nr_group_create_ex": (I, [ctypes.POINTER(P), I, I, ctypes.POINTER(P)]),
        "nr_group_synchronize": (I, [P]),
        "nr_group_layout": (I, [I, I, I, I, I, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]),
        "nr_group_size": (I, [P]),
        "nr_group_render_batch": (I, [P, ctypes.POINTER(NRFrame), I, I, I, I, I, I, ctypes.POINTER(NRStats)]),
        "nr_shard_rows": (I, [I, I, I, I]),
        "nr_batch_frames_per_launch": (I, [I, I, I, I, I, I, I]),
        "nr_assemble_shards": (I, [P, P, ctypes.c_size_t, P, I, I, I, I, I]),
        "nr_mlp_forward": (I, [P, P, P, L64, I]),
        "nr_mlp_gradient": (I, [P, P, L64, P, P, P, I, ctypes.POINTER(NRStats)]),
        "nr_project_points": (I, [P, P, L64, ctypes.POINTER(NRProjectOpts), P, P, P, P, P, P, I,
                                  ctypes.POINTER(NRStats)]),
        "nr_layer_forward": (I, [P, I, P, P, L64, I]),
        "nr_camera": (I, [F, F, F, F, F, FP, FP]),
        "nr_camera_ex": (I, [F, F, F, F, F, I, FP, FP]),
        "nr_h5_read_keras": (I, [ctypes.c_char_p, I, IP, IP, FP, ctypes.c_size_t]),
        "nr_h5_open": (I, [ctypes.c_char_p, ctypes.POINTER(P)]),
        "nr_h5_close": (None, [P]),
        "nr_h5_root": (I, [P, ctypes.POINTER(ctypes.c_uint64)]),
        "nr_h5_object_type": (I, [P, ctypes.c_uint64, IP]),
        "nr_h5_num_members": (I, [P, ctypes.c_uint64, ctypes.POINTER(ctypes.c_size_t)]),
        "nr_h5_member": (I, [P, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                             ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_uint64)]),
        "nr_h5_dims": (I, [P, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), I, IP]),
        "nr_h5_read_f32": (I, [P, ctypes.c_uint64, FP, ctypes.c_size_t]),
        "nr_png_load": (I, [ctypes.c_char_p, ctypes.POINTER(ctypes.POINTER(ctypes.c_uint32)), IP, IP]),
        "nr_png_save": (I, [ctypes.c_char_p, P, I, I, I]),
        "nr_ppm_save": (I, [ctypes.c_char_p, P, I, I]),
        "nr_free": (None, [P]),
        "nr_set_profiling": (I, [P, I]),
        "nr_prof_collect": (I, [P, ctypes.POINTER(NRKernelProf)]),
        "nr_set_poll_interval": (I, [P, I]),
        "nr_set_schedule": (I, [P, I]),
        "nr_set_debug": (I, [P, I]),
        "nr_set_endgame": (I, [P, F]),
        "nr_pack_fp32_pruned": (I, [I, IP, ctypes.POINTER(FP), ctypes.POINTER(FP), I, FP, FP, ctypes.c_long,
                                    ctypes.POINTER(ctypes.c_long), IP, IP, IP, IP, IP, I]),
        "nr_set_prune": (I, [P, I]),
        "nr_prune_info": (I, [P, IP, IP, IP, IP, I]),
        "nr_prune_redos": (I, [P, ctypes.POINTER(ctypes.c_ulonglong)]),
        "nr_set_unit_skip": (I, [P, I]),
        "nr_unit_skip_counts": (I, [P, ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_ulonglong)]),
        "nr_pack_fp32_units": (I, [I, IP, ctypes.POINTER(FP), ctypes.POINTER(FP), FP, ctypes.c_long,
                                   ctypes.POINTER(ctypes.c_long), IP]),
        "nr_set_occupancy": (I, [P, I]),
        "nr_set_pixel_spread": (I, [P, I]),
        "nr_set_cost_probe": (I, [P, I, I]),
        "nr_set_wave_rays": (I, [P, I]),
        "nr_set_queue_shards": (I, [P, I]),
        "nr_set_layer_chunk": (I, [P, ctypes.c_long]),
        "nr_set_temporal_order": (I, [P, I]),
        "nr_dense_forward": (I, [P, P, P, I, I, I, P, P, L64, I]),
        "nr_debug_stamps": (I, [P, P, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
        "nr_compose_create": (I, [P, ctypes.POINTER(P), I, ctypes.POINTER(NRPart), I, ctypes.POINTER(P)]),
        "nr_compose_destroy": (I, [P]),
        "nr_compose_bound": (I, [ctypes.POINTER(NRPart), I, I, FP, FP]),
        "nr_compose_set_parts": (I, [P, ctypes.POINTER(NRPart), I]),
        "nr_compose_info": (I, [P, IP, IP, FP, FP]),
        "nr_compose_sample": (I, [P, P, L64, P, P, I, ctypes.POINTER(NRComposeStats)]),
        "nr_compose_trace_rays": (I, [P, P, P, L64, I, P, P, P, P, P, P, I, ctypes.POINTER(NRComposeStats)]),
        "nr_compose_gbuffer": (I, [P, I, I, I, P, P, P, P, P, P, I, ctypes.POINTER(NRComposeStats)]),
        "nr_compose_render": (I, [P, P, I, I, I, P, I, ctypes.POINTER(NRComposeStats)]),
        "nr_compose_render_lit": (I, [P, P, I, I, I, ctypes.POINTER(NRLight), P, P, P, P, I, ctypes.POINTER(NRComposeStats)]),
        "nr_compose_sample_grid": (I, [P, FP, FP, IP, P, P, I, ctypes.POINTER(NRComposeStats)]),
        "nr_compose_extract_mesh": (I, [P, FP, FP, IP, F, P, P, P, L64, P, L64, ctypes.POINTER(L64), ctypes.POINTER(L64), I,
                                        ctypes.POINTER(NRComposeStats)]),
        "nr_compose_extract_mesh_sparse": (I, [P, FP, FP, IP, F, I, F, P, P, P, P, L64, P, L64, ctypes.POINTER(L64),
                                               ctypes.POINTER(L64), ctypes.POINTER(L64), I, ctypes.POINTER(NRComposeStats)]),
        "nr_fit_create": (I, [P, I, IP, ctypes.POINTER(FP), ctypes.POINTER(FP), ctypes.POINTER(NRFitOpts), ctypes.POINTER(P)]),
        "nr_fit_destroy": (I, [P]),
        "nr_fit_num_params": (I, [P, ctypes.POINTER(L64)]),
        "nr_fit_gradient": (I, [P, P, P, L64, P, P, P, I]),
        "nr_fit_run": (I, [P, P, P, L64, L64, P, I, ctypes.POINTER(NRStats)]),
        "nr_fit_weights": (I, [P, P, ctypes.POINTER(L64)]),
        "nr_obj_load": (I, [ctypes.c_char_p, ctypes.POINTER(FP), ctypes.POINTER(L64), ctypes.POINTER(IP), ctypes.POINTER(L64)]),
        "nr_trimesh_normals": (I, [P, L64, P, L64, P, IP]),
        "nr_trimesh_create": (I, [P, P, L64, P, L64, I, ctypes.POINTER(P)]),
        "nr_trimesh_destroy": (I, [P]),
        "nr_trimesh_info": (I, [P, ctypes.POINTER(L64), ctypes.POINTER(L64), ctypes.POINTER(L64), IP, FP, FP, IP]),
        "nr_trimesh_distance": (I, [P, P, L64, P, P, P, P, I, I, ctypes.POINTER(NRStats)]),
        "nr_mesh_hierarchy": (I, [P, L64, P, L64, I, ctypes.POINTER(FP), ctypes.POINTER(L64), ctypes.POINTER(IP),
                                  ctypes.POINTER(L64), ctypes.POINTER(FP), IP]),
        "nr_mesh_winding": (I, [P, P, L64, ctypes.c_float, P, P, I, I, ctypes.POINTER(NRStats)]),
        "nr_mesh_trace_rays": (I, [P, P, P, L64, ctypes.c_float, ctypes.c_float, P, P, P, P, P, P, I, I,
                                   ctypes.POINTER(NRStats)]),
        "nr_mesh_gbuffer": (I, [P, I, I, P, P, P, P, P, P, I, I, ctypes.POINTER(NRStats)]),
        "nr_mesh_render": (I, [P, P, I, I, I, I, ctypes.POINTER(NRStats)]),
        "nr_mesh_area_table": (I, [P, L64, P, L64, I, ctypes.POINTER(ctypes.POINTER(ctypes.c_uint32)), ctypes.POINTER(L64),
                                   ctypes.POINTER(L64)]),
        "nr_mesh_sample": (I, [P, ctypes.POINTER(NRSampleOpts), P, P, P, I, ctypes.POINTER(NRStats)]),
        "nr_points_order": (I, [P, P, L64, I, FP, FP, ctypes.c_uint64, P, P, I, ctypes.POINTER(NRStats)]),
        "nr_mesh_fit_samples": (I, [P, ctypes.POINTER(NRSampleOpts), P, P, I, ctypes.POINTER(NRStats)]),
        "nr_mesh_sample_grid": (I, [P, FP, FP, IP, I, F, I, P, I, ctypes.POINTER(NRStats)]),
        "nr_mesh_remesh": (I, [P, FP, FP, IP, F, I, F, P, P, L64, P, L64, ctypes.POINTER(L64), ctypes.POINTER(L64), I,
                                  ctypes.POINTER(NRStats)]),
        "nr_mesh_remesh_sparse": (I, [P, FP, FP, IP, F, I, F, I, F, P, P, P, L64, P, L64, ctypes.POINTER(L64),
                                         ctypes.POINTER(L64), ctypes.POINTER(L64), I, ctypes.POINTER(NRStats)]),
        "nr_mesh_create_device": (I, [P, P, L64, P, L64, I, ctypes.POINTER(P), ctypes.POINTER(NRStats)]),
        "nr_mesh_download": (I, [P, P, P, P, P, P, ctypes.POINTER(L64), ctypes.POINTER(L64)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(rc, ctx=None):
    if rc != NR_OK:
        msg = lib().nr_last_error(ctx)
        raise NRError(rc, msg.decode() if msg else "")
    return rc
