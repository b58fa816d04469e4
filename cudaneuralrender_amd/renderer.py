"""Python host side of the renderer: a thin object wrapper over the C ABI.

Mirrors the reference's host flow (src/main.cpp:636-678 -> generateSingleImage
:404-468): load the network (NeuralNetwork::load), optionally a matcap
(Image::loadPNG), copyStaticSettings, updateViewMatrices + copyViewMatrices, then
render_kernel.  All compute runs in libnr.so on the GPU.
"""
import ctypes

import numpy as np

from ._lib import (NR_AA_CONTRAST_DEFAULT, NR_AA_MODE, NR_COLOR_FACING, NR_COLOR_MATCAP, NR_DEVICE, NR_GROUP_ASYNC,
                   NR_GROUP_COPY, NR_HOST, NR_PRECISION, NR_SCENE, NR_SCHEDULE, NRFrame, NRKernelProf, NRLight, NRProjectOpts,
                   NRStats, check, lib)
from ._lib import NR_PART_OP, NRComposeStats, NRFitOpts, NRPart
from ._lib import NR_MESH_RAY_ANY, NR_MESH_RAY_SMOOTH, NR_TRIMESH_BRUTE
from ._lib import NR_ORDER, NR_SAMPLE_SIGN, NRSampleOpts

_FP = ctypes.POINTER(ctypes.c_float)


def _fptr(a):
    return a.ctypes.data_as(_FP)


def _iptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


CAMERA_MODES = {"f64": 0, "eigen": 1}


def camera(rx=0.0, ry=0.0, zoom=2.0, tx=0.0, ty=0.0, mode="f64"):
    """updateViewMatrices (main.cpp:207-222): returns (inv_view[12], normal[16]) float32.

    ``zoom`` is the value of the reference's ``-z`` flag (default 2): the eye sits at
    R * (tx, ty, zoom)... i.e. viewTranslation = (tx, ty, -zoom).  ``mode`` "f64": double
    arithmetic rounded once (nr_camera); "eigen": the reference's float Eigen expression restated
    (nr_camera_ex NR_CAMERA_EIGEN)."""
    iv = np.zeros(12, np.float32)
    nm = np.zeros(16, np.float32)
    check(lib().nr_camera_ex(rx, ry, zoom, tx, ty, CAMERA_MODES[mode], _fptr(iv), _fptr(nm)))
    return iv, nm


def read_keras_h5(path):
    """NeuralNetwork::load's reader (neuralNetwork.cpp:85-151) without a device:
    returns (dims, [kernel (in, out)], [bias (out,)])."""
    L = lib()
    nl = ctypes.c_int(0)
    check(L.nr_h5_read_keras(path.encode(), 0, ctypes.byref(nl), None, None, 0))
    dims = (ctypes.c_int * (nl.value + 1))()
    check(L.nr_h5_read_keras(path.encode(), nl.value, ctypes.byref(nl), dims, None, 0))
    dims = list(dims)
    total = sum(dims[i] * dims[i + 1] + dims[i + 1] for i in range(nl.value))
    buf = np.zeros(total, np.float32)
    check(L.nr_h5_read_keras(path.encode(), nl.value, ctypes.byref(nl), None, _fptr(buf), total))
    kernels, biases, off = [], [], 0
    for i in range(nl.value):
        n = dims[i] * dims[i + 1]
        kernels.append(buf[off:off + n].reshape(dims[i], dims[i + 1]).copy())
        off += n
        biases.append(buf[off:off + dims[i + 1]].copy())
        off += dims[i + 1]
    return dims, kernels, biases


def load_png(path):
    """Image::loadPNG (image.cu:36-65): (h, w) uint32 packed a<<24|b<<16|g<<8|r."""
    L = lib()
    p = ctypes.POINTER(ctypes.c_uint32)()
    w, h = ctypes.c_int(0), ctypes.c_int(0)
    check(L.nr_png_load(path.encode(), ctypes.byref(p), ctypes.byref(w), ctypes.byref(h)))
    try:
        arr = np.ctypeslib.as_array(p, shape=(h.value * w.value,)).copy().reshape(h.value, w.value)
    finally:
        L.nr_free(ctypes.cast(p, ctypes.c_void_p))
    return arr


def save_png(path, img, flip=True):
    """Image::savePNG (image.cu:67-110); flip=True is the reference's 180-degree rotation."""
    img = np.ascontiguousarray(img, dtype=np.uint32)
    check(lib().nr_png_save(path.encode(), img.ctypes.data, img.shape[1], img.shape[0], int(flip)))


def save_ppm(path, img):
    img = np.ascontiguousarray(img, dtype=np.uint32)
    check(lib().nr_ppm_save(path.encode(), img.ctypes.data, img.shape[1], img.shape[0]))


def save_obj(path, vertices, triangles, normals=None):
    """nr_obj_save: a Wavefront OBJ of the mesh (V [nv, 3] float32, T [nt, 3] int32, optional per-vertex
    normals [nv, 3]); floats are printed with %.9g, which round-trips float32."""
    V = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    T = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
    N = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    if N is not None and N.shape != V.shape:
        raise ValueError(f"normals {N.shape} and vertices {V.shape} differ")
    check(lib().nr_obj_save(str(path).encode(), V.ctypes.data, V.shape[0], None if N is None else N.ctypes.data,
                            T.ctypes.data, T.shape[0]))


def load_obj(path):
    """nr_obj_load: (V [nv, 3] float32, F [nt, 3] int32) of a Wavefront OBJ -- `v` and `f` records, 1-based or
    negative indices, i/t/n corners, polygons as fans from their first corner."""
    L = lib()
    vp, tp = _FP(), ctypes.POINTER(ctypes.c_int)()
    nv, nt = ctypes.c_long(0), ctypes.c_long(0)
    check(L.nr_obj_load(str(path).encode(), ctypes.byref(vp), ctypes.byref(nv), ctypes.byref(tp), ctypes.byref(nt)))
    try:
        V = np.ctypeslib.as_array(vp, shape=(nv.value * 3,)).copy() if nv.value else np.zeros(0, np.float32)
        T = np.ctypeslib.as_array(tp, shape=(nt.value * 3,)).copy() if nt.value else np.zeros(0, np.int32)
    finally:
        L.nr_free(ctypes.cast(vp, ctypes.c_void_p))
        L.nr_free(ctypes.cast(tp, ctypes.c_void_p))
    return V.reshape(-1, 3).astype(np.float32, copy=False), T.reshape(-1, 3).astype(np.int32, copy=False)


def _mesh_arrays(vertices, triangles):
    V = np.ascontiguousarray(vertices, np.float32)
    T = np.ascontiguousarray(triangles, np.int32)
    if V.ndim != 2 or V.shape[1] != 3 or T.ndim != 2 or T.shape[1] != 3:
        raise ValueError(f"vertices must be [nv, 3] and triangles [nt, 3], got {V.shape} and {T.shape}")
    return V, T


def trimesh_normals(vertices, triangles):
    """nr_trimesh_normals: (table [nt, 7, 3] float32, closed) -- the angle-weighted pseudonormals of every
    triangle's face, edges AB, BC, CA and vertices A, B, C (not normalised), and whether the mesh is
    closed and consistently wound."""
    V, T = _mesh_arrays(vertices, triangles)
    table = np.zeros((T.shape[0], 7, 3), np.float32)
    closed = ctypes.c_int(0)
    check(lib().nr_trimesh_normals(V.ctypes.data, V.shape[0], T.ctypes.data, T.shape[0], table.ctypes.data,
                                   ctypes.byref(closed)))
    return table, bool(closed.value)


def trimesh_hierarchy(vertices, triangles, leaf=0):
    """nr_mesh_hierarchy: (nodes [nnodes, 8] float32, order [ntl] int32, moments [nnodes, 16] float32,
    depth) -- the tree nr_trimesh_create builds and uploads, without a GPU.  Words 3 and 7 of a node
    are int32 (nodes.view(np.int32)): first | -count of a leaf, left | right child of an inner node;
    order is the original index of the live triangle at each position."""
    V, T = _mesh_arrays(vertices, triangles)
    L = lib()
    np_, mp, op = _FP(), _FP(), ctypes.POINTER(ctypes.c_int)()
    nn, ntl, depth = ctypes.c_long(0), ctypes.c_long(0), ctypes.c_int(0)
    check(L.nr_mesh_hierarchy(V.ctypes.data, V.shape[0], T.ctypes.data, T.shape[0], int(leaf), ctypes.byref(np_),
                              ctypes.byref(nn), ctypes.byref(op), ctypes.byref(ntl), ctypes.byref(mp), ctypes.byref(depth)))
    try:
        nodes = np.ctypeslib.as_array(np_, shape=(nn.value, 8)).copy()
        moments = np.ctypeslib.as_array(mp, shape=(nn.value, 16)).copy()
        order = np.ctypeslib.as_array(op, shape=(ntl.value,)).copy() if ntl.value else np.zeros(0, np.int32)
    finally:
        for q in (np_, mp, op):
            L.nr_free(ctypes.cast(q, ctypes.c_void_p))
    return nodes.astype(np.float32, copy=False), order.astype(np.int32, copy=False), moments.astype(np.float32, copy=False), depth.value


def mesh_area_table(vertices, triangles, leaf=0):
    """nr_mesh_area_table: (thresholds [ntl] uint32, last) -- the table nr_mesh_sample picks triangles
    from, over the live triangles in trimesh_hierarchy's order, without a GPU; last = -1 for a mesh
    without area."""
    V, T = _mesh_arrays(vertices, triangles)
    L = lib()
    tp = ctypes.POINTER(ctypes.c_uint32)()
    ntl, last = ctypes.c_long(0), ctypes.c_long(0)
    check(L.nr_mesh_area_table(V.ctypes.data, V.shape[0], T.ctypes.data, T.shape[0], int(leaf), ctypes.byref(tp),
                               ctypes.byref(ntl), ctypes.byref(last)))
    try:
        thr = np.ctypeslib.as_array(tp, shape=(ntl.value,)).copy() if ntl.value else np.zeros(0, np.uint32)
    finally:
        L.nr_free(ctypes.cast(tp, ctypes.c_void_p))
    return thr.astype(np.uint32, copy=False), last.value


def _sample_opts(seed, n_surface, n_volume, sigma, lo, hi, sign="normal", beta=0.0):
    lo = np.broadcast_to(np.asarray(lo, np.float32), (3,))
    hi = np.broadcast_to(np.asarray(hi, np.float32), (3,))
    return NRSampleOpts(int(seed), int(n_surface), int(n_volume), float(sigma), (ctypes.c_float * 3)(*lo),
                        (ctypes.c_float * 3)(*hi), NR_SAMPLE_SIGN[sign], float(beta))


def _lattice(origin, step, dims):
    """(origin, step, dims) as the C arrays of the lattice calls"""
    o = np.ascontiguousarray(origin, np.float32).reshape(3)
    s = np.ascontiguousarray(step, np.float32).reshape(3)
    d = (ctypes.c_int * 3)(*[int(v) for v in dims])
    return o, s, d


def pack_x3(dims, kernels, biases):
    """The library's fp32x3 pack of a fused-shape network (nr_pack_x3; host only): (a_ops uint16,
    floats float32, ok).  For the test oracle's emulation of the fp32x3 MLP (the bf16/fp16 tracers'
    normals)."""
    L = lib()
    nl = len(kernels)
    d = (ctypes.c_int * (nl + 1))(*dims)
    ks = [np.ascontiguousarray(k, np.float32) for k in kernels]
    bs = [np.ascontiguousarray(b, np.float32) for b in biases]
    kp = (_FP * nl)(*[_fptr(k) for k in ks])
    bp = (_FP * nl)(*[_fptr(b) for b in bs])
    na, nf, ok = ctypes.c_long(0), ctypes.c_long(0), ctypes.c_int(0)
    check(L.nr_pack_x3(nl, d, kp, bp, None, 0, None, 0, ctypes.byref(na), ctypes.byref(nf), ctypes.byref(ok)))
    a = np.zeros(na.value, np.uint16)
    f = np.zeros(nf.value, np.float32)
    check(L.nr_pack_x3(nl, d, kp, bp, a.ctypes.data, na.value, f.ctypes.data, nf.value, ctypes.byref(na),
                       ctypes.byref(nf), ctypes.byref(ok)))
    return a, f, ok.value


def pack_fp32_units(dims, kernels, biases):
    """The unit pack of a fused-shape network (nr_pack_fp32_units; host only) as float32, or None
    when it is refused (layout: csrc/nr_internal.h pack_fp32_units)."""
    L = lib()
    nl = len(kernels)
    d = (ctypes.c_int * (nl + 1))(*dims)
    ks_ = [np.ascontiguousarray(k, np.float32) for k in kernels]
    bs = [np.ascontiguousarray(b, np.float32) for b in biases]
    kp = (_FP * nl)(*[_fptr(k) for k in ks_])
    bp = (_FP * nl)(*[_fptr(b) for b in bs])
    n, hp = ctypes.c_long(0), ctypes.c_int(0)
    check(L.nr_pack_fp32_units(nl, d, kp, bp, None, 0, ctypes.byref(n), ctypes.byref(hp)))
    if not hp.value:
        return None
    pack = np.zeros(n.value, np.float32)
    check(L.nr_pack_fp32_units(nl, d, kp, bp, _fptr(pack), n.value, ctypes.byref(n), ctypes.byref(hp)))
    return pack


def pack_fp32_pruned(dims, kernels, biases, mode=1):
    """The library's fp32 packs of a fused-shape network (nr_pack_fp32_pruned; host only): a dict
    with full (float32), clamp, and -- None / empty when the scaled pack is refused -- pruned
    (float32), cand [nrelu], ks [nrelu] and order [nrelu][32] (position -> unit)."""
    L = lib()
    nl = len(kernels)
    d = (ctypes.c_int * (nl + 1))(*dims)
    ks_ = [np.ascontiguousarray(k, np.float32) for k in kernels]
    bs = [np.ascontiguousarray(b, np.float32) for b in biases]
    kp = (_FP * nl)(*[_fptr(k) for k in ks_])
    bp = (_FP * nl)(*[_fptr(b) for b in bs])
    n, cl, hp = ctypes.c_long(0), ctypes.c_int(0), ctypes.c_int(0)
    args = (nl, d, kp, bp, int(mode))
    check(L.nr_pack_fp32_pruned(*args, None, None, 0, ctypes.byref(n), ctypes.byref(cl), ctypes.byref(hp), None, None,
                                None, 0))
    nrelu = nl - 1
    full, pruned = np.zeros(n.value, np.float32), np.zeros(n.value, np.float32)
    cand, ks, order = np.zeros(nrelu, np.int32), np.zeros(nrelu, np.int32), np.zeros((nrelu, 32), np.int32)
    check(L.nr_pack_fp32_pruned(*args, _fptr(full), _fptr(pruned), n.value, ctypes.byref(n), ctypes.byref(cl),
                                ctypes.byref(hp), _iptr(cand), _iptr(ks), _iptr(order), nrelu))
    if not hp.value:
        return {"full": full, "clamp": cl.value, "pruned": None, "cand": cand[:0], "ks": ks[:0], "order": order[:0]}
    return {"full": full, "clamp": cl.value, "pruned": pruned, "cand": cand, "ks": ks, "order": order}


def shard_rows(H, band, nshards, shard):
    return lib().nr_shard_rows(H, band, nshards, shard)


def group_layout(W, H, band, n, nframes):
    """nr_group_layout: (shard_px, per_rank) of nr_group_render_batch's gather buffer."""
    a, b = ctypes.c_size_t(), ctypes.c_size_t()
    check(lib().nr_group_layout(W, H, band, n, nframes, ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def batch_frames_per_launch(W, H, band, nshards, shard, nframes, queue_shards=8):
    """Frames nr_render_batch puts in one k_trace launch (0: the shard overflows the
    32-bit pixel queue even for one frame)."""
    return lib().nr_batch_frames_per_launch(W, H, band, nshards, shard, nframes, queue_shards)


def assemble_shards(shards, W, H, band, nshards):
    """Host re-interleave of gathered shards (list or stacked array, each padded to a
    common stride) into the full frame."""
    stride = max(shard_rows(H, band, nshards, s) for s in range(nshards)) * W
    buf = np.zeros((nshards, stride), np.uint32)
    for s, sh in enumerate(shards):
        a = np.asarray(sh, np.uint32).reshape(-1)
        buf[s, :a.size] = a
    out = np.zeros((H, W), np.uint32)
    check(lib().nr_assemble_shards(None, buf.ctypes.data, stride, out.ctypes.data, W, H, band, nshards, NR_HOST))
    return out


class Renderer:
    """One renderer context per GPU (nr_ctx)."""

    def __init__(self, device=0):
        self._L = lib()
        self._ctx = ctypes.c_void_p()
        check(self._L.nr_create(device, ctypes.byref(self._ctx)))
        self.device = device

    # -- lifecycle
    def close(self):
        if self._ctx:
            self._L.nr_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        return check(rc, self._ctx)

    # -- network
    def load_h5(self, path):
        self._chk(self._L.nr_load_h5(self._ctx, path.encode()))
        return self

    def load_mlp(self, dims, kernels, biases):
        nl = len(kernels)
        d = (ctypes.c_int * (nl + 1))(*dims)
        ks = [np.ascontiguousarray(k, np.float32) for k in kernels]
        bs = [np.ascontiguousarray(b, np.float32) for b in biases]
        kp = (_FP * nl)(*[_fptr(k) for k in ks])
        bp = (_FP * nl)(*[_fptr(b) for b in bs])
        self._chk(self._L.nr_load_mlp(self._ctx, nl, d, kp, bp))
        return self

    def mlp_info(self):
        nl, nw, nb = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        dims = (ctypes.c_int * 64)()
        self._chk(self._L.nr_mlp_info(self._ctx, ctypes.byref(nl), dims, ctypes.byref(nw), ctypes.byref(nb)))
        return {"nlayers": nl.value, "dims": list(dims[:nl.value + 1]), "weights": nw.value, "biases": nb.value}

    def set_precision(self, precision):
        self._chk(self._L.nr_set_precision(self._ctx, NR_PRECISION[precision] if isinstance(precision, str) else precision))
        return self

    # -- settings
    def set_view(self, inv_view, normal, frame=0):
        iv = np.ascontiguousarray(inv_view, np.float32).reshape(12)
        nm = np.ascontiguousarray(normal, np.float32).reshape(16)
        self._chk(self._L.nr_set_view(self._ctx, _fptr(iv), _fptr(nm), int(frame)))
        return self

    def set_camera(self, rx=0.0, ry=0.0, zoom=2.0, frame=0):
        iv, nm = camera(rx, ry, zoom)
        return self.set_view(iv, nm, frame)

    def set_static(self, color_type=NR_COLOR_FACING, num_inputs=3):
        self._chk(self._L.nr_set_static(self._ctx, int(color_type), int(num_inputs)))
        return self

    def set_scene(self, scene):
        self._chk(self._L.nr_set_scene(self._ctx, NR_SCENE[scene] if isinstance(scene, str) else int(scene)))
        return self

    def set_matcap(self, rgba):
        m = np.ascontiguousarray(rgba, np.uint32)
        self._chk(self._L.nr_set_matcap(self._ctx, m.ctypes.data, m.shape[1], m.shape[0]))
        return self

    def set_stream(self, stream_ptr=None, own=False):
        """Issue work on `stream_ptr` (a hipStream_t as int; 0/None = HIP's null stream,
        e.g. torch.cuda.current_stream().cuda_stream), or on the private stream (own=True)."""
        self._chk(self._L.nr_set_stream(self._ctx, ctypes.c_void_p(stream_ptr) if stream_ptr else None, int(own)))
        return self

    def set_profiling(self, on=True):
        self._chk(self._L.nr_set_profiling(self._ctx, int(on)))

    def prof_collect(self):
        p = NRKernelProf()
        self._chk(self._L.nr_prof_collect(self._ctx, ctypes.byref(p)))
        return p.as_dict()

    def set_schedule(self, schedule):
        """"persistent" (one k_trace launch per frame, default), "wavefront" (one
        k_march launch per iteration) or "layered" (one dense-layer launch per layer per
        iteration, replayed as a hipGraph; networks of other shapes always use it)."""
        self._chk(self._L.nr_set_schedule(self._ctx, NR_SCHEDULE[schedule] if isinstance(schedule, str) else schedule))
        return self

    def set_occupancy(self, blocks_per_cu):
        self._chk(self._L.nr_set_occupancy(self._ctx, int(blocks_per_cu)))
        return self

    def set_pixel_spread(self, group_blocks):
        """Persistent schedule: deal each group of `group_blocks` 8x8 blocks pixel-major
        (0 = block-major; -1 = automatic, the default: 16 for one-frame launches, 0 for
        nr_render_batch launches of 4 or more frames)."""
        self._chk(self._L.nr_set_pixel_spread(self._ctx, int(group_blocks)))
        return self

    def set_cost_probe(self, max_steps, rays_per_wave=16):
        """Persistent schedule: probe each 8x8 block's centre ray (capped at max_steps
        iterations) before the frame and dispense blocks longest-first (0 = off)."""
        self._chk(self._L.nr_set_cost_probe(self._ctx, int(max_steps), int(rays_per_wave)))
        return self

    def set_wave_rays(self, rays):
        """Persistent schedule: at most `rays` (1-64) rays per wave at once; 0 = automatic (the
        default: 64, or 32 for an fp32 launch whose pixels fill at most 2x its waves' slots)."""
        self._chk(self._L.nr_set_wave_rays(self._ctx, int(rays)))
        return self

    def set_queue_shards(self, n):
        """Persistent schedule: number of pixel-queue counters (power of two <= 64)."""
        self._chk(self._L.nr_set_queue_shards(self._ctx, int(n)))
        return self

    def set_layer_chunk(self, points=0):
        """Layered schedule: points per dense-layer launch (0 = auto)."""
        self._chk(self._L.nr_set_layer_chunk(self._ctx, int(points)))
        return self

    def set_temporal_order(self, on=True):
        self._chk(self._L.nr_set_temporal_order(self._ctx, int(on)))
        return self

    def set_debug(self, flags):
        self._chk(self._L.nr_set_debug(self._ctx, int(flags)))
        return self

    def set_endgame(self, tau):
        """nr_set_endgame: bf16/fp16 rays whose 16-bit MLP output falls below tau finish their
        march in fp32x3 (default NR_ENDGAME_DEFAULT = 1e-3; 0 = the pure 16-bit march)."""
        self._chk(self._L.nr_set_endgame(self._ctx, float(tau)))
        return self

    def set_prune(self, mode):
        """nr_set_prune: the batched fp32 tracer's skipping of never-firing hidden units: 0 off,
        1 default, 2 test mode (four candidates per layer whatever they do).  Same frames and
        statistics in every mode."""
        self._chk(self._L.nr_set_prune(self._ctx, int(mode)))
        return self

    def prune_info(self):
        """nr_prune_info: {cand [nrelu], ks [nrelu], order [nrelu][32]} of the loaded network's
        pruned fp32 pack (empty arrays: none)."""
        n = ctypes.c_int(0)
        self._chk(self._L.nr_prune_info(self._ctx, ctypes.byref(n), None, None, None, 0))
        cand, ks, order = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32), np.zeros((n.value, 32), np.int32)
        self._chk(self._L.nr_prune_info(self._ctx, ctypes.byref(n), _iptr(cand), _iptr(ks), _iptr(order), n.value))
        return {"cand": cand, "ks": ks, "order": order}

    def set_unit_skip(self, on):
        """nr_set_unit_skip: the batched fp32 tracer's one-instruction-per-unit form, which skips
        the units that are +0 at every point of a wave (default on; it runs while the prune mode
        is 1).  Same images and statistics either way."""
        self._chk(self._L.nr_set_unit_skip(self._ctx, int(bool(on))))
        return self

    def unit_skip_counts(self):
        """nr_unit_skip_counts: (issued, skipped) of the last render_batch -- the unit instructions
        its waves came to, and those of them that were not executed."""
        a, b = ctypes.c_ulonglong(0), ctypes.c_ulonglong(0)
        self._chk(self._L.nr_unit_skip_counts(self._ctx, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def prune_redos(self):
        """nr_prune_redos: wave evaluations the last render_batch redid on the full fp32 pack."""
        v = ctypes.c_ulonglong(0)
        self._chk(self._L.nr_prune_redos(self._ctx, ctypes.byref(v)))
        return int(v.value)

    def debug_stamps(self):
        """Per-wave stamps of the last k_trace: {start, queue drained, end (100 MHz ticks),
        iterations after drain << 32 | iterations, shader-clock cycles in refill, shading,
        MLP, scene, step, within refill: reservation, bulk generation, dealing (bf16/fp16),
        after the drain: cycles in refill + shading + step, MLP, scene, and iterations with at
        most 4 rays}."""
        n = ctypes.c_size_t()
        self._chk(self._L.nr_debug_stamps(self._ctx, None, 0, ctypes.byref(n)))
        buf = np.zeros((n.value, 16), np.uint64)
        self._chk(self._L.nr_debug_stamps(self._ctx, buf.ctypes.data, buf.size, ctypes.byref(n)))
        return buf

    def set_poll_interval(self, every):
        self._chk(self._L.nr_set_poll_interval(self._ctx, int(every)))

    def synchronize(self):
        self._chk(self._L.nr_synchronize(self._ctx))

    # -- hot path
    def render(self, W, H, max_steps=6000, with_stats=True):
        out = np.zeros((H, W), np.uint32)
        st = NRStats()
        self._chk(self._L.nr_render(self._ctx, out.ctypes.data, W, H, max_steps, NR_HOST,
                                    ctypes.byref(st) if with_stats else None))
        return (out, st.as_dict()) if with_stats else out

    def render_device(self, out_ptr, W, H, max_steps=6000, with_stats=False):
        """Render into a device buffer (e.g. a torch tensor's data_ptr())."""
        st = NRStats()
        self._chk(self._L.nr_render(self._ctx, ctypes.c_void_p(out_ptr), W, H, max_steps, NR_DEVICE,
                                    ctypes.byref(st) if with_stats else None))
        return st.as_dict() if with_stats else None

    @staticmethod
    def _frames(cams, outs):
        fr = (NRFrame * len(cams))()
        for i, (cam, o) in enumerate(zip(cams, outs)):
            iv, nm = cam[0], cam[1]
            fr[i].inv_view[:] = [float(v) for v in np.asarray(iv, np.float32).reshape(-1)]
            fr[i].normal[:] = [float(v) for v in np.asarray(nm, np.float32).reshape(-1)]
            fr[i].frame = int(cam[2]) if len(cam) > 2 else 0
            fr[i].out = o
        return fr

    def render_batch(self, W, H, cams, max_steps=6000, band=8, nshards=1, shard=0, with_stats=True):
        """nr_render_batch to host images: cams = [(inv_view, normal[, frame]), ...].
        Returns the list of (rows, W) images (and the summed stats)."""
        rows = shard_rows(H, band, nshards, shard)
        outs = [np.zeros((rows, W), np.uint32) for _ in cams]
        fr = self._frames(cams, [o.ctypes.data for o in outs])
        st = NRStats()
        self._chk(self._L.nr_render_batch(self._ctx, fr, len(cams), W, H, band, nshards, shard, max_steps, NR_HOST,
                                          ctypes.byref(st) if with_stats else None))
        return (outs, st.as_dict()) if with_stats else outs

    def render_batch_device(self, out_ptrs, W, H, cams, max_steps=6000, band=8, nshards=1, shard=0,
                            with_stats=False):
        """nr_render_batch into device buffers (one per camera)."""
        fr = self._frames(cams, list(out_ptrs))
        st = NRStats()
        self._chk(self._L.nr_render_batch(self._ctx, fr, len(cams), W, H, band, nshards, shard, max_steps, NR_DEVICE,
                                          ctypes.byref(st) if with_stats else None))
        return st.as_dict() if with_stats else None

    def render_shard(self, W, H, band, nshards, shard, max_steps=6000, with_stats=True):
        rows = shard_rows(H, band, nshards, shard)
        out = np.zeros((rows, W), np.uint32)
        st = NRStats()
        self._chk(self._L.nr_render_shard(self._ctx, out.ctypes.data, W, H, band, nshards, shard, max_steps,
                                          NR_HOST, ctypes.byref(st) if with_stats else None))
        return (out, st.as_dict()) if with_stats else out

    def render_shard_device(self, out_ptr, W, H, band, nshards, shard, max_steps=6000, with_stats=False):
        st = NRStats()
        self._chk(self._L.nr_render_shard(self._ctx, ctypes.c_void_p(out_ptr), W, H, band, nshards, shard,
                                          max_steps, NR_DEVICE, ctypes.byref(st) if with_stats else None))
        return st.as_dict() if with_stats else None

    def assemble_device(self, src_ptr, stride, dst_ptr, W, H, band, nshards):
        self._chk(self._L.nr_assemble_shards(self._ctx, ctypes.c_void_p(src_ptr), stride, ctypes.c_void_p(dst_ptr),
                                             W, H, band, nshards, NR_DEVICE))

    # -- ray queries / geometry buffers
    @staticmethod
    def _query_outputs(shape, normals):
        return {"status": np.zeros(shape, np.int32), "steps": np.zeros(shape, np.int32),
                "t": np.zeros(shape, np.float32), "position": np.zeros(shape + (3,), np.float32),
                "normal": np.zeros(shape + (3,), np.float32) if normals else None}

    def trace_rays(self, origins, dirs, max_steps=6000, normals=True, with_stats=False):
        """nr_trace_rays on host arrays: march the rays p = origins[i] + t * dirs[i] (dirs as given,
        not normalised) as nr_render marches a pixel ray.  Returns a dict of numpy arrays: status
        (NR_RAY_*), steps, t, position (n, 3) and normal (n, 3); normals=False skips the normal
        evaluations and leaves "normal" out (shadow / occlusion rays).  Always the fp32 MLP."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError(f"origins {o.shape} and dirs {d.shape} differ")
        n = o.shape[0]
        out = self._query_outputs((n,), normals)
        st = NRStats()
        self._chk(self._L.nr_trace_rays(self._ctx, o.ctypes.data, d.ctypes.data, n, int(max_steps),
                                        *[a.ctypes.data if a is not None else None for a in out.values()], NR_HOST,
                                        ctypes.byref(st) if with_stats else None))
        if not normals:
            del out["normal"]
        return (out, st.as_dict()) if with_stats else out

    def trace_rays_device(self, origins_ptr, dirs_ptr, n, max_steps=6000, status_ptr=None, steps_ptr=None, t_ptr=None,
                          position_ptr=None, normal_ptr=None, with_stats=False):
        """nr_trace_rays on device buffers (e.g. torch tensors' data_ptr(): float32 [n, 3] rays,
        int32 status / steps, float32 t, [n, 3] position / normal); None = that output is not wanted.
        Runs on the context's stream (set_stream) and, without stats, returns without waiting."""
        vp = [ctypes.c_void_p(p) if p else None
              for p in (origins_ptr, dirs_ptr, status_ptr, steps_ptr, t_ptr, position_ptr, normal_ptr)]
        st = NRStats()
        self._chk(self._L.nr_trace_rays(self._ctx, vp[0], vp[1], int(n), int(max_steps), *vp[2:], NR_DEVICE,
                                        ctypes.byref(st) if with_stats else None))
        return st.as_dict() if with_stats else None

    def render_gbuffer(self, W, H, max_steps=6000, normals=True, with_stats=False):
        """nr_render_gbuffer: the trace_rays outputs for the W x H pixel rays of the current view,
        shaped (H, W) and (H, W, 3); status == NR_RAY_HIT exactly where render() colours the pixel."""
        out = self._query_outputs((H, W), normals)
        st = NRStats()
        self._chk(self._L.nr_render_gbuffer(self._ctx, W, H, int(max_steps),
                                            *[a.ctypes.data if a is not None else None for a in out.values()], NR_HOST,
                                            ctypes.byref(st) if with_stats else None))
        if not normals:
            del out["normal"]
        return (out, st.as_dict()) if with_stats else out

    # -- adaptive supersampled antialiasing
    def _render_aa(self, out, W, H, samples, mode, contrast, max_steps, loc, with_stats):
        st = NRStats()
        edges = ctypes.c_long(0)
        self._chk(self._L.nr_render_aa(self._ctx, out, int(W), int(H), int(samples), NR_AA_MODE[mode], int(contrast),
                                       int(max_steps), loc, ctypes.byref(edges),
                                       ctypes.byref(st) if with_stats else None))
        d = st.as_dict() if with_stats else {}
        d["edge_pixels"] = edges.value
        return d

    def render_aa(self, W, H, samples=2, mode="adaptive", contrast=NR_AA_CONTRAST_DEFAULT, max_steps=6000,
                  with_stats=True):
        """nr_render_aa: the W x H frame with its edge pixels (mode "adaptive": those whose
        8-neighbourhood differs by more than ``contrast`` in some channel; "full": every pixel) box-
        filtered from samples x samples sub-pixel rays -- the pixels of render()'s samples W x samples H
        frame.  Alpha becomes coverage, colours come out premultiplied.  Always the fp32 MLP.  Returns
        (image, stats) with stats["edge_pixels"]."""
        out = np.zeros((H, W), np.uint32)
        st = self._render_aa(out.ctypes.data, W, H, samples, mode, contrast, max_steps, NR_HOST, with_stats)
        return (out, st) if with_stats else out

    def render_aa_device(self, out_ptr, W, H, samples=2, mode="adaptive", contrast=NR_AA_CONTRAST_DEFAULT,
                         max_steps=6000, with_stats=False):
        """nr_render_aa into a device buffer of W * H uint32 (e.g. a torch tensor's data_ptr()), on the
        context's stream (set_stream).  Returns the stats dict when asked for, else the edge-pixel count."""
        st = self._render_aa(ctypes.c_void_p(out_ptr), W, H, samples, mode, contrast, max_steps, NR_DEVICE, with_stats)
        return st if with_stats else st["edge_pixels"]

    # -- ambient occlusion and soft shadows
    @staticmethod
    def _light(light_dir, shadow_steps, shadow_bias, shadow_k, ao_step, ao_strength, ambient):
        lt = NRLight()
        lt.dir[:] = [float(v) for v in np.asarray(light_dir, np.float32).reshape(3)]
        lt.shadow_steps = int(shadow_steps)
        lt.shadow_bias, lt.shadow_k = float(shadow_bias), float(shadow_k)
        lt.ao_step, lt.ao_strength, lt.ambient = float(ao_step), float(ao_strength), float(ambient)
        return lt

    def render_lit(self, W, H, light_dir, shadow_steps=64, shadow_bias=0.01, shadow_k=8.0, ao_step=0.02,
                   ao_strength=2.0, ambient=0.3, max_steps=6000, buffers=False, with_stats=False):
        """nr_render_lit: render()'s fp32 frame lit by one directional light (light_dir: from the
        surface towards the light, used as given), every coloured pixel scaled by
        ao * (ambient + (1 - ambient) * shadow * max(dot(n, light_dir), 0)): ao from four field samples
        along the normal, shadow from a sphere-traced ray towards the light (soft for shadow_k > 0).
        Always the fp32 MLP.  Returns the (H, W) uint32 image; buffers=True: (image, ao, shadow) with
        the two (H, W) float32 factors; with_stats=True appends the stats dict."""
        out = np.zeros((H, W), np.uint32)
        ao = np.zeros((H, W), np.float32) if buffers else None
        sh = np.zeros((H, W), np.float32) if buffers else None
        lt = self._light(light_dir, shadow_steps, shadow_bias, shadow_k, ao_step, ao_strength, ambient)
        st = NRStats()
        self._chk(self._L.nr_render_lit(self._ctx, out.ctypes.data, int(W), int(H), int(max_steps), ctypes.byref(lt),
                                        ao.ctypes.data if buffers else None, sh.ctypes.data if buffers else None,
                                        NR_HOST, ctypes.byref(st) if with_stats else None))
        res = (out, ao, sh) if buffers else (out,)
        if with_stats:
            res += (st.as_dict(),)
        return res if len(res) > 1 else out

    def render_lit_device(self, out_ptr, W, H, light_dir, shadow_steps=64, shadow_bias=0.01, shadow_k=8.0, ao_step=0.02,
                          ao_strength=2.0, ambient=0.3, max_steps=6000, ao_ptr=None, shadow_ptr=None, with_stats=False):
        """nr_render_lit into device buffers (e.g. torch tensors' data_ptr(): W * H uint32 for the
        frame, W * H float32 for ao and shadow; None = that output is not wanted, but not all three),
        on the context's stream (set_stream).  Without stats it returns without waiting."""
        vp = [ctypes.c_void_p(p) if p else None for p in (out_ptr, ao_ptr, shadow_ptr)]
        lt = self._light(light_dir, shadow_steps, shadow_bias, shadow_k, ao_step, ao_strength, ambient)
        st = NRStats()
        self._chk(self._L.nr_render_lit(self._ctx, vp[0], int(W), int(H), int(max_steps), ctypes.byref(lt), vp[1], vp[2],
                                        NR_DEVICE, ctypes.byref(st) if with_stats else None))
        return st.as_dict() if with_stats else None

    # -- volume sampling / isosurface extraction
    def sample_grid(self, origin, step, dims, with_stats=False):
        """nr_sample_grid: the scene's distance at the lattice points origin + (i, j, k) * step,
        dims = (nx, ny, nz), generated in the kernel.  Returns float32 [nz, ny, nx].  Always the
        fp32 MLP."""
        o, s, d = _lattice(origin, step, dims)
        out = np.zeros((d[2], d[1], d[0]), np.float32)
        st = NRStats()
        self._chk(self._L.nr_sample_grid(self._ctx, _fptr(o), _fptr(s), d, out.ctypes.data, NR_HOST,
                                         ctypes.byref(st) if with_stats else None))
        return (out, st.as_dict()) if with_stats else out

    def sample_grid_device(self, sdf_ptr, origin, step, dims, with_stats=False):
        """nr_sample_grid into a device buffer of nx * ny * nz float32 (e.g. a torch tensor's
        data_ptr()).  Runs on the context's stream (set_stream) and, without stats, returns without
        waiting."""
        o, s, d = _lattice(origin, step, dims)
        st = NRStats()
        self._chk(self._L.nr_sample_grid(self._ctx, _fptr(o), _fptr(s), d, ctypes.c_void_p(sdf_ptr), NR_DEVICE,
                                         ctypes.byref(st) if with_stats else None))
        return st.as_dict() if with_stats else None

    def mesh_grid(self, sdf, origin, step, iso=0.0):
        """nr_mesh_grid: marching tetrahedra over the lattice values sdf [nz, ny, nx] (any values; no
        network needed).  Returns (V [nv, 3] float32, T [nt, 3] int32): a count-only call first, then
        the buffers are allocated."""
        sdf = np.ascontiguousarray(sdf, np.float32)
        if sdf.ndim != 3:
            raise ValueError(f"sdf must be [nz, ny, nx], got {sdf.shape}")
        o, s, d = _lattice(origin, step, sdf.shape[::-1])
        nv, nt = ctypes.c_long(0), ctypes.c_long(0)

        def call(V, T):
            return self._L.nr_mesh_grid(self._ctx, sdf.ctypes.data, _fptr(o), _fptr(s), d, float(iso),
                                        None if V is None else V.ctypes.data, 0 if V is None else V.shape[0],
                                        None if T is None else T.ctypes.data, 0 if T is None else T.shape[0],
                                        ctypes.byref(nv), ctypes.byref(nt), NR_HOST)

        self._chk(call(None, None))
        V, T = np.zeros((nv.value, 3), np.float32), np.zeros((nt.value, 3), np.int32)
        if nv.value:
            self._chk(call(V, T))
        return V, T

    def extract_mesh(self, origin, step, dims, iso=0.0, normals=True, with_stats=False):
        """nr_extract_mesh: sample the lattice on the device and mesh it.  Returns a dict with
        "vertices" [nv, 3] float32, "triangles" [nt, 3] int32 and, with normals=True, "normals"
        [nv, 3] (the normalised tetrahedral gradient at each vertex).  The count-only call comes first
        (it samples the lattice too), then the buffers are allocated."""
        o, s, d = _lattice(origin, step, dims)
        nv, nt = ctypes.c_long(0), ctypes.c_long(0)
        st = NRStats()

        def call(V, N, T):
            return self._L.nr_extract_mesh(self._ctx, _fptr(o), _fptr(s), d, float(iso),
                                           None if V is None else V.ctypes.data, None if N is None else N.ctypes.data,
                                           0 if V is None else V.shape[0], None if T is None else T.ctypes.data,
                                           0 if T is None else T.shape[0], ctypes.byref(nv), ctypes.byref(nt), NR_HOST,
                                           ctypes.byref(st) if with_stats else None)

        self._chk(call(None, None, None))
        V, T = np.zeros((nv.value, 3), np.float32), np.zeros((nt.value, 3), np.int32)
        N = np.zeros((nv.value, 3), np.float32) if normals else None
        if nv.value:
            self._chk(call(V, N, T))
        out = {"vertices": V, "triangles": T}
        if normals:
            out["normals"] = N
        return (out, st.as_dict()) if with_stats else out

    def _sparse_band(self, step, brick, band):
        """band=None: the brick's diagonal, computed in double and rounded to f32 -- the bound that is
        sound for a field with gradient at most 1."""
        if band is not None:
            return float(band)
        return float(np.float32(np.sqrt(sum((float(brick) * float(x)) ** 2 for x in step))))

    def extract_mesh_sparse(self, origin, step, dims, iso=0.0, brick=8, band=None, normals=True, keys=True,
                            with_stats=False):
        """nr_extract_mesh_sparse: nr_extract_mesh restricted to the bricks of brick^3 cells that have
        a corner within `band` of iso (or a sign change, or a NaN) -- for lattices too large to sample
        densely.  band=None is the brick's diagonal; too small a band leaves holes.  Returns a dict with
        "vertices" [nv, 3] float32, "triangles" [nt, 3] int32, "active_bricks" and, as asked, "normals"
        [nv, 3] and "keys" [nv] int64 (index * 7 + slot: np.argsort(keys) is the dense mesh's vertex
        order).  The count-only call comes first, then the buffers are allocated."""
        o, s, d = _lattice(origin, step, dims)
        bandf = self._sparse_band(s, brick, band)
        nv, nt, na = ctypes.c_long(0), ctypes.c_long(0), ctypes.c_long(0)
        st = NRStats()

        def call(V, N, K, T):
            return self._L.nr_extract_mesh_sparse(
                self._ctx, _fptr(o), _fptr(s), d, float(iso), int(brick), bandf,
                None if V is None else V.ctypes.data, None if N is None else N.ctypes.data,
                None if K is None else K.ctypes.data, 0 if V is None else V.shape[0],
                None if T is None else T.ctypes.data, 0 if T is None else T.shape[0],
                ctypes.byref(nv), ctypes.byref(nt), ctypes.byref(na), NR_HOST, ctypes.byref(st) if with_stats else None)

        self._chk(call(None, None, None, None))
        V, T = np.zeros((nv.value, 3), np.float32), np.zeros((nt.value, 3), np.int32)
        N = np.zeros((nv.value, 3), np.float32) if normals else None
        K = np.zeros((nv.value,), np.int64) if keys else None
        if nv.value:
            self._chk(call(V, N, K, T))
        out = {"vertices": V, "triangles": T, "active_bricks": na.value}
        if normals:
            out["normals"] = N
        if keys:
            out["keys"] = K
        return (out, st.as_dict()) if with_stats else out

    def extract_mesh_sparse_device(self, origin, step, dims, vertices_ptr, v_cap, triangles_ptr, t_cap, iso=0.0, brick=8,
                                   band=None, normals_ptr=None, keys_ptr=None, with_stats=False):
        """nr_extract_mesh_sparse into device buffers (e.g. torch tensors' data_ptr(): v_cap x 3
        float32 vertices and normals, v_cap int64 keys, t_cap x 3 int32 triangles; both vertices_ptr
        and triangles_ptr None: count only), on the context's stream (set_stream).  Returns
        (nv, nt, active_bricks), with the stats dict appended with_stats=True; short capacities raise
        NRError with nothing written."""
        o, s, d = _lattice(origin, step, dims)
        vp = [ctypes.c_void_p(p) if p else None for p in (vertices_ptr, normals_ptr, keys_ptr, triangles_ptr)]
        nv, nt, na = ctypes.c_long(0), ctypes.c_long(0), ctypes.c_long(0)
        st = NRStats()
        self._chk(self._L.nr_extract_mesh_sparse(
            self._ctx, _fptr(o), _fptr(s), d, float(iso), int(brick), self._sparse_band(s, brick, band), vp[0], vp[1], vp[2],
            int(v_cap), vp[3], int(t_cap), ctypes.byref(nv), ctypes.byref(nt), ctypes.byref(na), NR_DEVICE,
            ctypes.byref(st) if with_stats else None))
        res = (nv.value, nt.value, na.value)
        return res + (st.as_dict(),) if with_stats else res

    def mlp_forward(self, X):
        X = np.ascontiguousarray(X, np.float32)
        info = self.mlp_info()
        n = X.shape[0]
        Y = np.zeros((n, info["dims"][-1]), np.float32)
        self._chk(self._L.nr_mlp_forward(self._ctx, X.ctypes.data, Y.ctypes.data, n, NR_HOST))
        return Y

    def mlp_forward_device(self, x_ptr, y_ptr, n):
        self._chk(self._L.nr_mlp_forward(self._ctx, ctypes.c_void_p(x_ptr), ctypes.c_void_p(y_ptr), n, NR_DEVICE))

    def mlp_gradient(self, X, value=True, grad=True, normal=False, with_stats=False):
        """nr_mlp_gradient on a host array X [n, dims[0]]: the network's value [n] (nr_mlp_forward's
        fp32 bits), its exact gradient [n, dims[0]] by one backward pass and the normalised gradient
        [n, 3] of the first three inputs.  Returns a dict of the numpy arrays asked for ("value",
        "grad", "normal"; at least one).  Always the fp32 MLP."""
        X = np.ascontiguousarray(X, np.float32)
        if X.ndim != 2:
            raise ValueError(f"X must be [n, inputs], got {X.shape}")
        n, in0 = X.shape
        out = {}
        if value:
            out["value"] = np.zeros((n,), np.float32)
        if grad:
            out["grad"] = np.zeros((n, in0), np.float32)
        if normal:
            out["normal"] = np.zeros((n, 3), np.float32)
        ptr = [out[k].ctypes.data if k in out else None for k in ("value", "grad", "normal")]
        st = NRStats()
        self._chk(self._L.nr_mlp_gradient(self._ctx, X.ctypes.data, n, *ptr, NR_HOST,
                                          ctypes.byref(st) if with_stats else None))
        return (out, st.as_dict()) if with_stats else out

    def mlp_gradient_device(self, x_ptr, n, value_ptr=None, grad_ptr=None, normal_ptr=None, with_stats=False):
        """nr_mlp_gradient on device buffers (e.g. torch tensors' data_ptr(): float32 X [n, dims[0]],
        value [n], grad [n, dims[0]], normal [n, 3]); None = that output is not wanted.  Runs on the
        context's stream (set_stream) and, without stats, returns without waiting."""
        vp = [ctypes.c_void_p(p) if p else None for p in (x_ptr, value_ptr, grad_ptr, normal_ptr)]
        st = NRStats()
        self._chk(self._L.nr_mlp_gradient(self._ctx, vp[0], int(n), *vp[1:], NR_DEVICE,
                                          ctypes.byref(st) if with_stats else None))
        return st.as_dict() if with_stats else None

    PROJECT_OUTPUTS = ("position", "value", "normal", "distance", "iters", "status")

    def project_points(self, X, iso=0.0, tol=1e-5, max_step=0.25, max_iters=32, outputs=PROJECT_OUTPUTS, with_stats=False):
        """nr_project_points on a host array X [n, dims[0]]: every point moved onto the level set
        {network value == iso} by Newton steps along the analytic gradient, in one launch.  Returns a
        dict of the numpy arrays named in outputs (at least one of "position" [n, 3], "value" [n],
        "normal" [n, 3], "distance" [n], "iters" [n] int32, "status" [n] int32 = NR_PROJ_*).  max_step:
        the longest step in world units, 0 = unlimited.  Always the fp32 MLP."""
        X = np.ascontiguousarray(X, np.float32)
        if X.ndim != 2:
            raise ValueError(f"X must be [n, inputs], got {X.shape}")
        unknown = [k for k in outputs if k not in self.PROJECT_OUTPUTS]
        if unknown:
            raise ValueError(f"unknown outputs {unknown}")
        n = X.shape[0]
        shape = {"position": ((n, 3), np.float32), "value": ((n,), np.float32), "normal": ((n, 3), np.float32),
                 "distance": ((n,), np.float32), "iters": ((n,), np.int32), "status": ((n,), np.int32)}
        out = {k: np.zeros(*shape[k]) for k in self.PROJECT_OUTPUTS if k in outputs}
        ptr = [out[k].ctypes.data if k in out else None for k in self.PROJECT_OUTPUTS]
        opts = NRProjectOpts(float(iso), float(tol), float(max_step), int(max_iters))
        st = NRStats()
        self._chk(self._L.nr_project_points(self._ctx, X.ctypes.data, n, ctypes.byref(opts), *ptr, NR_HOST,
                                            ctypes.byref(st) if with_stats else None))
        return (out, st.as_dict()) if with_stats else out

    def project_points_device(self, x_ptr, n, iso=0.0, tol=1e-5, max_step=0.25, max_iters=32, position_ptr=None,
                              value_ptr=None, normal_ptr=None, distance_ptr=None, iters_ptr=None, status_ptr=None,
                              with_stats=False):
        """nr_project_points on device buffers (e.g. torch tensors' data_ptr(): float32 X [n, dims[0]],
        position [n, 3], value [n], normal [n, 3], distance [n], int32 iters [n], status [n]); None =
        that output is not wanted.  Runs on the context's stream (set_stream) and, without stats,
        returns without waiting."""
        vp = [ctypes.c_void_p(p) if p else None
              for p in (x_ptr, position_ptr, value_ptr, normal_ptr, distance_ptr, iters_ptr, status_ptr)]
        opts = NRProjectOpts(float(iso), float(tol), float(max_step), int(max_iters))
        st = NRStats()
        self._chk(self._L.nr_project_points(self._ctx, vp[0], int(n), ctypes.byref(opts), *vp[1:], NR_DEVICE,
                                            ctypes.byref(st) if with_stats else None))
        return st.as_dict() if with_stats else None

    def layer_forward(self, layer, A):
        A = np.ascontiguousarray(A, np.float32)
        info = self.mlp_info()
        Z = np.zeros((A.shape[0], info["dims"][layer + 1]), np.float32)
        self._chk(self._L.nr_layer_forward(self._ctx, layer, A.ctypes.data, Z.ctypes.data, A.shape[0], NR_HOST))
        return Z

    def order_points(self, X=None, n=None, mode="morton", lo=-1.0, hi=1.0, seed=0, sorted_points=False, with_stats=False):
        """nr_points_order on a host array X [n, 3] (mode "shuffle": X may be None, n given): perm [n] int32,
        the stable ascending order of the points' 30-bit Morton codes in the box [lo, hi] or of the
        seed's Philox keys -- np.argsort(keys, kind="stable") -- and with sorted_points also X[perm].
        Needs no network."""
        if X is not None:
            X = np.ascontiguousarray(X, np.float32)
            if X.ndim != 2 or X.shape[1] != 3:
                raise ValueError(f"X must be [n, 3], got {X.shape}")
            n = X.shape[0]
        n = int(n)
        lo3 = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, np.float32), (3,)))
        hi3 = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, np.float32), (3,)))
        perm = np.zeros(max(n, 0), np.int32)
        out = np.zeros((max(n, 0), 3), np.float32) if sorted_points else None
        st = NRStats()
        self._chk(self._L.nr_points_order(self._ctx, None if X is None else X.ctypes.data, n, NR_ORDER[mode], _fptr(lo3), _fptr(hi3),
                                          int(seed), perm.ctypes.data, out.ctypes.data if sorted_points else None, NR_HOST,
                                          ctypes.byref(st) if with_stats else None))
        res = (perm, out) if sorted_points else perm
        return (res, st.as_dict()) if with_stats else res

    def order_points_device(self, x_ptr, n, perm_ptr, mode="morton", lo=-1.0, hi=1.0, seed=0, sorted_ptr=None, with_stats=False):
        """nr_points_order on device buffers (float32 X [n, 3] or None, int32 perm [n], float32 sorted [n, 3] or
        None); runs on the renderer's stream and, without stats, returns without waiting."""
        lo3 = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, np.float32), (3,)))
        hi3 = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, np.float32), (3,)))
        vp = [ctypes.c_void_p(p) if p else None for p in (x_ptr, perm_ptr, sorted_ptr)]
        st = NRStats()
        self._chk(self._L.nr_points_order(self._ctx, vp[0], int(n), NR_ORDER[mode], _fptr(lo3), _fptr(hi3), int(seed), vp[1],
                                          vp[2], NR_DEVICE, ctypes.byref(st) if with_stats else None))
        return st.as_dict() if with_stats else None


__all__ = ["Renderer", "camera", "pack_x3", "read_keras_h5", "load_png", "save_png", "save_ppm", "save_obj", "shard_rows",
           "assemble_shards", "NR_COLOR_FACING", "NR_COLOR_MATCAP"]


class Group:
    """nr_group: renderers on distinct GPUs of one process joined by one RCCL communicator.
    render_batch splits every frame into row-band shards (renderer r renders shard r), checks
    every shard's status, gathers the shards to the first renderer's GPU in one RCCL call and
    re-interleaves them there (include/neural_render.h nr_group_render_batch)."""

    def __init__(self, renderers, copy=False, asynchronous=False):
        """copy: NR_GROUP_COPY (hipMemcpyPeerAsync transfers; renderers may share a GPU);
        asynchronous: NR_GROUP_ASYNC (a call returns with its gather enqueued: synchronize())."""
        self._L = lib()
        self.renderers = list(renderers)
        arr = (ctypes.c_void_p * len(self.renderers))(*[r._ctx.value for r in self.renderers])
        self._g = ctypes.c_void_p()
        flags = (NR_GROUP_COPY if copy else 0) | (NR_GROUP_ASYNC if asynchronous else 0)
        check(self._L.nr_group_create_ex(arr, len(self.renderers), flags, ctypes.byref(self._g)))

    def synchronize(self):
        check(self._L.nr_group_synchronize(self._g))
        return self

    def close(self):
        if self._g:
            self._L.nr_group_destroy(self._g)
            self._g = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def size(self):
        return self._L.nr_group_size(self._g)

    def render_batch(self, W, H, cams, max_steps=6000, band=1, with_stats=True):
        """Full frames (H, W) on the host for cams = [(inv_view, normal[, frame]), ...]."""
        outs = [np.zeros((H, W), np.uint32) for _ in cams]
        fr = Renderer._frames(cams, [o.ctypes.data for o in outs])
        st = NRStats()
        check(self._L.nr_group_render_batch(self._g, fr, len(cams), W, H, band, max_steps, NR_HOST,
                                            ctypes.byref(st) if with_stats else None))
        return (outs, st.as_dict()) if with_stats else outs

    def render_batch_device(self, out_ptrs, W, H, cams, max_steps=6000, band=1, with_stats=False):
        """Full frames into device buffers on the first renderer's GPU."""
        fr = Renderer._frames(cams, list(out_ptrs))
        st = NRStats()
        check(self._L.nr_group_render_batch(self._g, fr, len(cams), W, H, band, max_steps, NR_DEVICE,
                                            ctypes.byref(st) if with_stats else None))
        return st.as_dict() if with_stats else None


def make_parts(parts):
    """A list of parts as the C array of nr_part.  Each part is a dict (or a tuple in this order):
    net, op ("union" / "subtract" or NR_PART_*; default union), rot (3 x 3, local -> world; default
    identity), pos (default 0) and scale (default 1)."""
    arr = (NRPart * len(parts))()
    for a, p in zip(arr, parts):
        if not isinstance(p, dict):
            p = dict(zip(("net", "op", "rot", "pos", "scale"), p))
        op = p.get("op", 0)
        a.net = int(p.get("net", 0))
        a.op = NR_PART_OP[op] if isinstance(op, str) else int(op)
        a.rot[:] = [float(v) for v in np.asarray(p.get("rot", np.eye(3)), np.float32).reshape(9)]
        a.pos[:] = [float(v) for v in np.asarray(p.get("pos", (0, 0, 0)), np.float32).reshape(3)]
        a.scale = float(np.float32(p.get("scale", 1.0)))
    return arr


def compose_bound(parts, nnets):
    """nr_compose_bound (host only): the parts checked as create checks them, and the world bound
    (center float32 [3], radius float32) they give."""
    arr = make_parts(parts)
    c = np.zeros(3, np.float32)
    r = ctypes.c_float(0)
    check(lib().nr_compose_bound(arr, len(arr), int(nnets), _fptr(c), ctypes.byref(r)))
    return c, np.float32(r.value)


class Composition:
    """nr_compose: up to 4 networks (Renderers with a fused network loaded) placed as up to 16 parts
    and combined by union / subtraction, traced as one scene.  `owner` is the Renderer whose device,
    stream, view, frame number, colour settings and matcap every call uses; the nets may be closed
    afterwards, the composition must be closed before its owner."""

    def __init__(self, owner, nets, parts):
        self._L = lib()
        self.owner = owner
        self._c = ctypes.c_void_p()
        nets = list(nets)
        self.nnets = len(nets)
        arr = (ctypes.c_void_p * max(len(nets), 1))(*[r._ctx.value for r in nets])
        pa = make_parts(parts)
        owner._chk(self._L.nr_compose_create(owner._ctx, arr, len(nets), pa, len(pa), ctypes.byref(self._c)))

    def close(self):
        if self._c:
            # (the C object reaches through its owner: after an owner closed first it is left alone)
            if self.owner._ctx:
                self._L.nr_compose_destroy(self._c)
            self._c = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        return check(rc, self.owner._ctx)

    def set_parts(self, parts):
        """New transforms, ops or part count; the packs are not uploaded again."""
        pa = make_parts(parts)
        self._chk(self._L.nr_compose_set_parts(self._c, pa, len(pa)))
        return self

    def info(self):
        nn, npart, c, r = ctypes.c_int(0), ctypes.c_int(0), np.zeros(3, np.float32), ctypes.c_float(0)
        self._chk(self._L.nr_compose_info(self._c, ctypes.byref(nn), ctypes.byref(npart), _fptr(c), ctypes.byref(r)))
        return {"nets": nn.value, "parts": npart.value, "center": c, "radius": np.float32(r.value)}

    def sample(self, points, with_stats=False):
        """The field at host points [n, 3]: {"value": float32 [n], "owner": int32 [n]}."""
        P = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n = P.shape[0]
        out = {"value": np.zeros(n, np.float32), "owner": np.zeros(n, np.int32)}
        st = NRComposeStats()
        self._chk(self._L.nr_compose_sample(self._c, P.ctypes.data, n, out["value"].ctypes.data, out["owner"].ctypes.data,
                                            NR_HOST, ctypes.byref(st) if with_stats else None))
        return (out, st.as_dict()) if with_stats else out

    @staticmethod
    def _outputs(shape, normals):
        out = Renderer._query_outputs(shape, normals)
        out["part"] = np.zeros(shape, np.int32)
        return out

    def trace_rays(self, origins, dirs, max_steps=6000, normals=True, with_stats=False):
        """nr_compose_trace_rays on host arrays: Renderer.trace_rays' dict plus "part", the part that
        owns each hit (-1 for any other status)."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError(f"origins {o.shape} and dirs {d.shape} differ")
        n = o.shape[0]
        out = self._outputs((n,), normals)
        st = NRComposeStats()
        self._chk(self._L.nr_compose_trace_rays(self._c, o.ctypes.data, d.ctypes.data, n, int(max_steps),
                                                *[a.ctypes.data if a is not None else None for a in out.values()], NR_HOST,
                                                ctypes.byref(st) if with_stats else None))
        if not normals:
            del out["normal"]
        return (out, st.as_dict()) if with_stats else out

    def trace_rays_device(self, origins_ptr, dirs_ptr, n, max_steps=6000, status_ptr=None, steps_ptr=None, t_ptr=None,
                          position_ptr=None, normal_ptr=None, part_ptr=None, with_stats=False):
        """nr_compose_trace_rays on device buffers, on the owner's stream (Renderer.trace_rays_device)."""
        vp = [ctypes.c_void_p(p) if p else None
              for p in (origins_ptr, dirs_ptr, status_ptr, steps_ptr, t_ptr, position_ptr, normal_ptr, part_ptr)]
        st = NRComposeStats()
        self._chk(self._L.nr_compose_trace_rays(self._c, vp[0], vp[1], int(n), int(max_steps), *vp[2:], NR_DEVICE,
                                                ctypes.byref(st) if with_stats else None))
        return st.as_dict() if with_stats else None

    def gbuffer(self, W, H, max_steps=6000, normals=True, with_stats=False):
        """nr_compose_gbuffer: the trace_rays outputs for the W x H pixel rays of the owner's view,
        shaped (H, W) and (H, W, 3)."""
        out = self._outputs((H, W), normals)
        st = NRComposeStats()
        self._chk(self._L.nr_compose_gbuffer(self._c, W, H, int(max_steps),
                                             *[a.ctypes.data if a is not None else None for a in out.values()], NR_HOST,
                                             ctypes.byref(st) if with_stats else None))
        if not normals:
            del out["normal"]
        return (out, st.as_dict()) if with_stats else out

    def gbuffer_device(self, W, H, max_steps=6000, status_ptr=None, steps_ptr=None, t_ptr=None, position_ptr=None,
                       normal_ptr=None, part_ptr=None, with_stats=False):
        vp = [ctypes.c_void_p(p) if p else None for p in (status_ptr, steps_ptr, t_ptr, position_ptr, normal_ptr, part_ptr)]
        st = NRComposeStats()
        self._chk(self._L.nr_compose_gbuffer(self._c, int(W), int(H), int(max_steps), *vp, NR_DEVICE,
                                             ctypes.byref(st) if with_stats else None))
        return st.as_dict() if with_stats else None

    def render(self, W, H, max_steps=6000, with_part=False, with_stats=True):
        """nr_compose_render: the (H, W) uint32 frame in the owner's colouring; with_part adds the
        (H, W) int32 owner map."""
        img = np.zeros((H, W), np.uint32)
        part = np.zeros((H, W), np.int32) if with_part else None
        st = NRComposeStats()
        self._chk(self._L.nr_compose_render(self._c, img.ctypes.data, W, H, int(max_steps),
                                            part.ctypes.data if with_part else None, NR_HOST,
                                            ctypes.byref(st) if with_stats else None))
        res = (img,) + ((part,) if with_part else ()) + ((st.as_dict(),) if with_stats else ())
        return res if len(res) > 1 else img

    # -- ambient occlusion and shadows cast between the parts
    def render_lit(self, W, H, light_dir, shadow_steps=64, shadow_bias=0.01, shadow_k=8.0, ao_step=0.02,
                   ao_strength=2.0, ambient=0.3, max_steps=6000, buffers=False, with_part=False, with_occluder=False,
                   with_stats=False):
        """nr_compose_render_lit: render()'s frame lit by one directional light as Renderer.render_lit
        lights a single network, with the occlusion and the shadow rays taken through the composed
        field: a part shades the others, a cut-out lies in the dark.  Returns the (H, W) uint32 image;
        buffers=True adds the (H, W) float32 ao and shadow, with_part the (H, W) int32 owner map,
        with_occluder the (H, W) int32 map of the part that blocked each pixel's light (-1: none),
        with_stats the stats dict, in this order."""
        out = np.zeros((H, W), np.uint32)
        ao = np.zeros((H, W), np.float32) if buffers else None
        sh = np.zeros((H, W), np.float32) if buffers else None
        part = np.zeros((H, W), np.int32) if with_part else None
        occ = np.zeros((H, W), np.int32) if with_occluder else None
        lt = Renderer._light(light_dir, shadow_steps, shadow_bias, shadow_k, ao_step, ao_strength, ambient)
        st = NRComposeStats()
        self._chk(self._L.nr_compose_render_lit(self._c, out.ctypes.data, int(W), int(H), int(max_steps), ctypes.byref(lt),
                                                *[a.ctypes.data if a is not None else None for a in (ao, sh, part, occ)],
                                                NR_HOST, ctypes.byref(st) if with_stats else None))
        res = (out,) + ((ao, sh) if buffers else ()) + ((part,) if with_part else ()) + ((occ,) if with_occluder else ())
        if with_stats:
            res += (st.as_dict(),)
        return res if len(res) > 1 else out

    def render_lit_device(self, out_ptr, W, H, light_dir, shadow_steps=64, shadow_bias=0.01, shadow_k=8.0, ao_step=0.02,
                          ao_strength=2.0, ambient=0.3, max_steps=6000, ao_ptr=None, shadow_ptr=None, part_ptr=None,
                          occluder_ptr=None, with_stats=False):
        """nr_compose_render_lit into device buffers (W * H uint32 for the frame, float32 for ao and
        shadow, int32 for part and occluder; None = that output is not wanted, but not all of out, ao
        and shadow), on the owner's stream.  Without stats it returns without waiting."""
        vp = [ctypes.c_void_p(p) if p else None for p in (out_ptr, ao_ptr, shadow_ptr, part_ptr, occluder_ptr)]
        lt = Renderer._light(light_dir, shadow_steps, shadow_bias, shadow_k, ao_step, ao_strength, ambient)
        st = NRComposeStats()
        self._chk(self._L.nr_compose_render_lit(self._c, vp[0], int(W), int(H), int(max_steps), ctypes.byref(lt), *vp[1:],
                                                NR_DEVICE, ctypes.byref(st) if with_stats else None))
        return st.as_dict() if with_stats else None

    # -- lattice sampling / isosurface extraction of the composed field
    def sample_grid(self, origin, step, dims, owner=False, with_stats=False):
        """nr_compose_sample_grid: the composed field at the lattice points origin + (i, j, k) * step,
        dims = (nx, ny, nz), generated in the kernel.  Returns float32 [nz, ny, nx]; with owner=True
        (value, owner int32 [nz, ny, nx])."""
        o, s, d = _lattice(origin, step, dims)
        val = np.zeros((d[2], d[1], d[0]), np.float32)
        own = np.zeros((d[2], d[1], d[0]), np.int32) if owner else None
        st = NRComposeStats()
        self._chk(self._L.nr_compose_sample_grid(self._c, _fptr(o), _fptr(s), d, val.ctypes.data,
                                                 own.ctypes.data if owner else None, NR_HOST,
                                                 ctypes.byref(st) if with_stats else None))
        res = (val,) + ((own,) if owner else ()) + ((st.as_dict(),) if with_stats else ())
        return res if len(res) > 1 else val

    def sample_grid_device(self, origin, step, dims, value_ptr=None, owner_ptr=None, with_stats=False):
        """nr_compose_sample_grid into device buffers of nx * ny * nz float32 / int32 (at least one), on
        the owner's stream."""
        o, s, d = _lattice(origin, step, dims)
        vp = [ctypes.c_void_p(p) if p else None for p in (value_ptr, owner_ptr)]
        st = NRComposeStats()
        self._chk(self._L.nr_compose_sample_grid(self._c, _fptr(o), _fptr(s), d, vp[0], vp[1], NR_DEVICE,
                                                 ctypes.byref(st) if with_stats else None))
        return st.as_dict() if with_stats else None

    def extract_mesh(self, origin, step, dims, iso=0.0, normals=True, part=False, with_stats=False):
        """nr_compose_extract_mesh: sample the composed field on the lattice and mesh it.  Returns
        Renderer.extract_mesh's dict ("vertices", "triangles", "normals" as asked) plus, with
        part=True, "part" [nv] int32: the part that owns the field at each vertex.  The count-only
        call comes first (it samples the lattice too), then the buffers are allocated."""
        o, s, d = _lattice(origin, step, dims)
        nv, nt = ctypes.c_long(0), ctypes.c_long(0)
        st = NRComposeStats()

        def call(V, N, P, T):
            return self._L.nr_compose_extract_mesh(
                self._c, _fptr(o), _fptr(s), d, float(iso), None if V is None else V.ctypes.data,
                None if N is None else N.ctypes.data, None if P is None else P.ctypes.data, 0 if V is None else V.shape[0],
                None if T is None else T.ctypes.data, 0 if T is None else T.shape[0], ctypes.byref(nv), ctypes.byref(nt),
                NR_HOST, ctypes.byref(st) if with_stats else None)

        self._chk(call(None, None, None, None))
        V, T = np.zeros((nv.value, 3), np.float32), np.zeros((nt.value, 3), np.int32)
        N = np.zeros((nv.value, 3), np.float32) if normals else None
        P = np.zeros((nv.value,), np.int32) if part else None
        if nv.value:
            self._chk(call(V, N, P, T))
        out = {"vertices": V, "triangles": T}
        if normals:
            out["normals"] = N
        if part:
            out["part"] = P
        return (out, st.as_dict()) if with_stats else out

    def extract_mesh_device(self, origin, step, dims, vertices_ptr, v_cap, triangles_ptr, t_cap, iso=0.0, normals_ptr=None,
                            part_ptr=None, with_stats=False):
        """nr_compose_extract_mesh into device buffers (v_cap x 3 float32 vertices and normals, v_cap
        int32 owners, t_cap x 3 int32 triangles; vertices_ptr and triangles_ptr both None: count only),
        on the owner's stream.  Returns (nv, nt), with the stats dict appended with_stats=True; short
        capacities raise NRError with nothing written."""
        o, s, d = _lattice(origin, step, dims)
        vp = [ctypes.c_void_p(p) if p else None for p in (vertices_ptr, normals_ptr, part_ptr, triangles_ptr)]
        nv, nt = ctypes.c_long(0), ctypes.c_long(0)
        st = NRComposeStats()
        self._chk(self._L.nr_compose_extract_mesh(self._c, _fptr(o), _fptr(s), d, float(iso), vp[0], vp[1], vp[2], int(v_cap),
                                                  vp[3], int(t_cap), ctypes.byref(nv), ctypes.byref(nt), NR_DEVICE,
                                                  ctypes.byref(st) if with_stats else None))
        res = (nv.value, nt.value)
        return res + (st.as_dict(),) if with_stats else res

    def extract_mesh_sparse(self, origin, step, dims, iso=0.0, brick=8, band=None, normals=True, part=False, keys=True,
                            with_stats=False):
        """nr_compose_extract_mesh_sparse: extract_mesh restricted to the bricks of brick^3 cells that
        have a corner within `band` of iso (or a sign change, or a NaN).  band=None is the brick's
        diagonal, as Renderer.extract_mesh_sparse; too small a band leaves holes.  Returns that
        method's dict ("vertices", "triangles", "active_bricks", "normals" and "keys" as asked) plus,
        with part=True, "part" [nv] int32."""
        o, s, d = _lattice(origin, step, dims)
        bandf = self.owner._sparse_band(s, brick, band)
        nv, nt, na = ctypes.c_long(0), ctypes.c_long(0), ctypes.c_long(0)
        st = NRComposeStats()

        def call(V, N, P, K, T):
            return self._L.nr_compose_extract_mesh_sparse(
                self._c, _fptr(o), _fptr(s), d, float(iso), int(brick), bandf,
                None if V is None else V.ctypes.data, None if N is None else N.ctypes.data,
                None if P is None else P.ctypes.data, None if K is None else K.ctypes.data, 0 if V is None else V.shape[0],
                None if T is None else T.ctypes.data, 0 if T is None else T.shape[0],
                ctypes.byref(nv), ctypes.byref(nt), ctypes.byref(na), NR_HOST, ctypes.byref(st) if with_stats else None)

        self._chk(call(None, None, None, None, None))
        V, T = np.zeros((nv.value, 3), np.float32), np.zeros((nt.value, 3), np.int32)
        N = np.zeros((nv.value, 3), np.float32) if normals else None
        P = np.zeros((nv.value,), np.int32) if part else None
        K = np.zeros((nv.value,), np.int64) if keys else None
        if nv.value:
            self._chk(call(V, N, P, K, T))
        out = {"vertices": V, "triangles": T, "active_bricks": na.value}
        if normals:
            out["normals"] = N
        if part:
            out["part"] = P
        if keys:
            out["keys"] = K
        return (out, st.as_dict()) if with_stats else out

    def extract_mesh_sparse_device(self, origin, step, dims, vertices_ptr, v_cap, triangles_ptr, t_cap, iso=0.0, brick=8,
                                   band=None, normals_ptr=None, part_ptr=None, keys_ptr=None, with_stats=False):
        """nr_compose_extract_mesh_sparse into device buffers, shaped like
        Renderer.extract_mesh_sparse_device with the v_cap int32 owners added.  Returns
        (nv, nt, active_bricks), with the stats dict appended with_stats=True."""
        o, s, d = _lattice(origin, step, dims)
        vp = [ctypes.c_void_p(p) if p else None for p in (vertices_ptr, normals_ptr, part_ptr, keys_ptr, triangles_ptr)]
        nv, nt, na = ctypes.c_long(0), ctypes.c_long(0), ctypes.c_long(0)
        st = NRComposeStats()
        self._chk(self._L.nr_compose_extract_mesh_sparse(
            self._c, _fptr(o), _fptr(s), d, float(iso), int(brick), self.owner._sparse_band(s, brick, band), vp[0], vp[1],
            vp[2], vp[3], int(v_cap), vp[4], int(t_cap), ctypes.byref(nv), ctypes.byref(nt), ctypes.byref(na), NR_DEVICE,
            ctypes.byref(st) if with_stats else None))
        res = (nv.value, nt.value, na.value)
        return res + (st.as_dict(),) if with_stats else res


class Fit:
    """nr_fit: a [3, 32, ..., 32, 1] network trained on the device -- the weight gradients of the plain
    or clamped L2 loss and Adam, bit for bit the arithmetic written in include/neural_render.h.
    `renderer` supplies the device and the stream (it needs no network); the initial kernels and
    biases are the caller's, in load_mlp's layout.  Close the fit before its renderer."""

    def __init__(self, renderer, dims, kernels, biases, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, clamp=0.0,
                 partials=0, grid=0):
        self._L = lib()
        self.owner = renderer
        self._f = ctypes.c_void_p()
        self.dims = [int(d) for d in dims]
        nl = len(kernels)
        d = (ctypes.c_int * (nl + 1))(*self.dims)
        ks = [np.ascontiguousarray(k, np.float32) for k in kernels]
        bs = [np.ascontiguousarray(b, np.float32) for b in biases]
        kp = (_FP * nl)(*[_fptr(k) for k in ks])
        bp = (_FP * nl)(*[_fptr(b) for b in bs])
        opts = NRFitOpts(lr, beta1, beta2, eps, clamp, int(partials), int(grid))
        renderer._chk(self._L.nr_fit_create(renderer._ctx, nl, d, kp, bp, ctypes.byref(opts), ctypes.byref(self._f)))
        cnt = ctypes.c_long(0)
        self._chk(self._L.nr_fit_num_params(self._f, ctypes.byref(cnt)))
        self.num_params = cnt.value

    def close(self):
        if self._f:
            # (the C object reaches through its owner: after an owner closed first it is left alone)
            if self.owner._ctx:
                self._L.nr_fit_destroy(self._f)
            self._f = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        return check(rc, self.owner._ctx)

    def _split(self, flat):
        K, B, q = [], [], 0
        for i, o in zip(self.dims[:-1], self.dims[1:]):
            K.append(flat[q:q + i * o].reshape(i, o).copy()); q += i * o
            B.append(flat[q:q + o].copy()); q += o
        return K, B

    @staticmethod
    def _xy(X, Y):
        X = np.ascontiguousarray(X, np.float32)
        Y = np.ascontiguousarray(Y, np.float32).reshape(-1)
        if X.ndim != 2 or X.shape[1] != 3 or len(Y) != len(X):
            raise ValueError(f"X must be [n, 3] and Y [n], got {X.shape} and {Y.shape}")
        return X, Y

    def gradient(self, X, Y, value=False):
        """nr_fit_gradient on host arrays: {"loss", "grad": (kernels, biases)[, "value"]}; the weights stay."""
        X, Y = self._xy(X, Y)
        n = len(X)
        loss = np.zeros(1, np.float32)
        flat = np.zeros(self.num_params, np.float32)
        val = np.zeros(n, np.float32) if value else None
        self._chk(self._L.nr_fit_gradient(self._f, X.ctypes.data, Y.ctypes.data, n, loss.ctypes.data, flat.ctypes.data,
                                          val.ctypes.data if value else None, NR_HOST))
        out = {"loss": loss[0], "grad": self._split(flat), "flat": flat}
        if value:
            out["value"] = val
        return out

    def gradient_device(self, x_ptr, y_ptr, n, loss_ptr=None, grad_ptr=None, value_ptr=None):
        """nr_fit_gradient on device buffers (float32 X [n, 3], Y [n], loss [1], grad [P], value [n]);
        runs on the renderer's stream and returns without waiting."""
        vp = [ctypes.c_void_p(p) if p else None for p in (x_ptr, y_ptr, loss_ptr, grad_ptr, value_ptr)]
        self._chk(self._L.nr_fit_gradient(self._f, vp[0], vp[1], int(n), vp[2], vp[3], vp[4], NR_DEVICE))

    def run(self, X, Y, batch, with_stats=False):
        """nr_fit_run on host arrays: len(X) / batch Adam steps; returns each step's loss before its update."""
        X, Y = self._xy(X, Y)
        n = len(X)
        loss = np.zeros(max(n // max(int(batch), 1), 1), np.float32)
        st = NRStats()
        self._chk(self._L.nr_fit_run(self._f, X.ctypes.data, Y.ctypes.data, n, int(batch), loss.ctypes.data, NR_HOST,
                                     ctypes.byref(st) if with_stats else None))
        return (loss, st.as_dict()) if with_stats else loss

    def run_device(self, x_ptr, y_ptr, n, batch, loss_ptr=None, with_stats=False):
        """nr_fit_run on device buffers (float32 X [n, 3], Y [n], loss [n / batch] or None): enqueues
        the steps on the renderer's stream and, without stats, returns without waiting."""
        st = NRStats()
        self._chk(self._L.nr_fit_run(self._f, ctypes.c_void_p(x_ptr), ctypes.c_void_p(y_ptr), int(n), int(batch),
                                     ctypes.c_void_p(loss_ptr) if loss_ptr else None, NR_DEVICE,
                                     ctypes.byref(st) if with_stats else None))
        return st.as_dict() if with_stats else None

    def weights(self):
        """(dims, kernels, biases, step): the master weights and the steps taken so far."""
        flat = np.zeros(self.num_params, np.float32)
        step = ctypes.c_long(0)
        self._chk(self._L.nr_fit_weights(self._f, flat.ctypes.data, ctypes.byref(step)))
        K, B = self._split(flat)
        return self.dims, K, B, step.value

    def load_into(self, renderer):
        """The current weights into `renderer` (nr_load_mlp builds every pack); returns the renderer."""
        dims, K, B, _ = self.weights()
        return renderer.load_mlp(dims, K, B)


class TriMesh:
    """nr_trimesh: a triangle mesh, its pseudonormals and a box hierarchy on the device, queried for the
    signed distance of points -- bit for bit the arithmetic written in include/neural_render.h.
    `renderer` supplies the device and the stream (it needs no network).  leaf: triangles per leaf of
    the hierarchy, 0 = 8.  build: "host" (nr_trimesh_create: the spatial-median tree, built on one host
    thread) or "device" (the arrays are uploaded and nr_mesh_create_device builds the Morton-ordered
    tree with kernels; from_device takes arrays that are on the device already).  Close the mesh before
    its renderer."""

    def __init__(self, renderer, vertices, triangles, leaf=0, build="host"):
        self._L = lib()
        self.owner = renderer
        self._m = ctypes.c_void_p()
        self.build_stats = None
        V, T = _mesh_arrays(vertices, triangles)
        if build == "host":
            renderer._chk(self._L.nr_trimesh_create(renderer._ctx, V.ctypes.data, V.shape[0], T.ctypes.data, T.shape[0],
                                                    int(leaf), ctypes.byref(self._m)))
        elif build == "device":
            import torch
            dev = torch.device("cuda", renderer.device)
            dV, dT = torch.from_numpy(V.copy()).to(dev), torch.from_numpy(T.copy()).to(dev)
            torch.cuda.synchronize(dev)
            self._create_device(dV.data_ptr(), V.shape[0], dT.data_ptr(), T.shape[0], leaf, False)
        else:
            raise ValueError(f"build must be 'host' or 'device', got {build!r}")

    def _create_device(self, vertices_ptr, nv, triangles_ptr, nt, leaf, with_stats):
        st = NRStats()
        self.owner._chk(self._L.nr_mesh_create_device(self.owner._ctx, ctypes.c_void_p(vertices_ptr), int(nv),
                                                         ctypes.c_void_p(triangles_ptr), int(nt), int(leaf),
                                                         ctypes.byref(self._m), ctypes.byref(st) if with_stats else None))
        self.build_stats = st.as_dict() if with_stats else None

    @classmethod
    def from_device(cls, renderer, vertices_ptr, nv, triangles_ptr, nt, leaf=0, with_stats=False):
        """nr_mesh_create_device on device buffers (float32 vertices [nv, 3], int32 triangles [nt, 3]),
        e.g. extract_mesh_device's: the mesh is built by kernels and nothing but two small records
        crosses to the host.  The buffers are read during the call only.  With with_stats the build's
        statistics are left in .build_stats."""
        self = cls.__new__(cls)
        self._L = lib()
        self.owner = renderer
        self._m = ctypes.c_void_p()
        self._create_device(vertices_ptr, nv, triangles_ptr, nt, leaf, with_stats)
        return self

    def download(self):
        """nr_mesh_download: {"nodes" [nnodes, 8], "order" [ntl] int32, "moments" [nnodes, 16], "table"
        [nt, 7, 3], "thresholds" [ntl] uint32, "ntl", "area_last"} -- what the object holds on the device,
        however it was built (words 3 and 7 of a node are int32, as trimesh_hierarchy's)."""
        info = self.info()
        ntl, last = ctypes.c_long(0), ctypes.c_long(0)
        self._chk(self._L.nr_mesh_download(self._m, None, None, None, None, None, ctypes.byref(ntl), ctypes.byref(last)))
        out = {"nodes": np.zeros((info["nodes"], 8), np.float32), "order": np.zeros(ntl.value, np.int32),
               "moments": np.zeros((info["nodes"], 16), np.float32), "table": np.zeros((info["nt"], 7, 3), np.float32),
               "thresholds": np.zeros(ntl.value, np.uint32)}
        self._chk(self._L.nr_mesh_download(self._m, *[out[k].ctypes.data if out[k].size else None
                                                         for k in ("nodes", "order", "moments", "table", "thresholds")],
                                              None, None))
        out["ntl"], out["area_last"] = ntl.value, last.value
        return out

    def close(self):
        if self._m:
            # (the C object reaches through its owner: after an owner closed first it is left alone)
            if self.owner._ctx:
                self._L.nr_trimesh_destroy(self._m)
            self._m = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        return check(rc, self.owner._ctx)

    def info(self):
        """{"nv", "nt", "nodes", "depth", "lo", "hi", "closed"}: the mesh, its hierarchy and its bound."""
        nv, nt, nodes = ctypes.c_long(0), ctypes.c_long(0), ctypes.c_long(0)
        depth, closed = ctypes.c_int(0), ctypes.c_int(0)
        lo, hi = np.zeros(3, np.float32), np.zeros(3, np.float32)
        self._chk(self._L.nr_trimesh_info(self._m, ctypes.byref(nv), ctypes.byref(nt), ctypes.byref(nodes),
                                          ctypes.byref(depth), _fptr(lo), _fptr(hi), ctypes.byref(closed)))
        return {"nv": nv.value, "nt": nt.value, "nodes": nodes.value, "depth": depth.value, "lo": lo, "hi": hi,
                "closed": bool(closed.value)}

    def distance(self, X, closest=False, tri=False, feature=False, brute=False, with_stats=False):
        """nr_trimesh_distance on a host array X [n, 3]: {"sdf" [n][, "closest" [n, 3], "tri" [n] int32,
        "feature" [n] int32]} -- negative inside a closed mesh whose triangles wind outward.  brute:
        every triangle, no hierarchy (the same bits).  Neighbours in space should be neighbours in X."""
        X = np.ascontiguousarray(X, np.float32)
        if X.ndim != 2 or X.shape[1] != 3:
            raise ValueError(f"X must be [n, 3], got {X.shape}")
        n = X.shape[0]
        out = {"sdf": np.zeros(n, np.float32)}
        if closest:
            out["closest"] = np.zeros((n, 3), np.float32)
        if tri:
            out["tri"] = np.zeros(n, np.int32)
        if feature:
            out["feature"] = np.zeros(n, np.int32)
        ptr = [out[k].ctypes.data if k in out else None for k in ("sdf", "closest", "tri", "feature")]
        st = NRStats()
        self._chk(self._L.nr_trimesh_distance(self._m, X.ctypes.data, n, *ptr, NR_TRIMESH_BRUTE if brute else 0, NR_HOST,
                                              ctypes.byref(st) if with_stats else None))
        return (out, st.as_dict()) if with_stats else out

    def distance_device(self, x_ptr, n, sdf_ptr=None, closest_ptr=None, tri_ptr=None, feature_ptr=None, brute=False,
                        with_stats=False):
        """nr_trimesh_distance on device buffers (float32 X [n, 3], sdf [n], closest [n, 3], int32 tri [n],
        feature [n]); None = that output is not wanted.  Runs on the renderer's stream and, without
        stats, returns without waiting."""
        vp = [ctypes.c_void_p(p) if p else None for p in (x_ptr, sdf_ptr, closest_ptr, tri_ptr, feature_ptr)]
        st = NRStats()
        self._chk(self._L.nr_trimesh_distance(self._m, vp[0], int(n), *vp[1:], NR_TRIMESH_BRUTE if brute else 0, NR_DEVICE,
                                              ctypes.byref(st) if with_stats else None))
        return st.as_dict() if with_stats else None

    def winding(self, X, beta=0.0, sdf=False, brute=False, with_stats=False):
        """nr_mesh_winding on a host array X [n, 3]: {"winding" [n][, "sdf" [n]]} -- the generalized
        winding number (1 inside a closed mesh that winds outward, 0 outside; w >= 0.5 is the inside
        test of a mesh that is open or overlaps itself) and, with sdf, nr_trimesh_distance's magnitude
        signed by that test.  beta: a node counts as far beyond beta radii, 0 = 2.0.  brute: every
        triangle, no expansion.  Neighbours in space should be neighbours in X."""
        X = np.ascontiguousarray(X, np.float32)
        if X.ndim != 2 or X.shape[1] != 3:
            raise ValueError(f"X must be [n, 3], got {X.shape}")
        n = X.shape[0]
        out = {"winding": np.zeros(n, np.float32)}
        if sdf:
            out["sdf"] = np.zeros(n, np.float32)
        st = NRStats()
        self._chk(self._L.nr_mesh_winding(self._m, X.ctypes.data, n, float(beta), out["winding"].ctypes.data,
                                          out["sdf"].ctypes.data if sdf else None, NR_TRIMESH_BRUTE if brute else 0,
                                          NR_HOST, ctypes.byref(st) if with_stats else None))
        return (out, st.as_dict()) if with_stats else out

    def winding_device(self, x_ptr, n, winding_ptr=0, sdf_ptr=0, beta=0.0, brute=False, with_stats=False):
        """nr_mesh_winding on device buffers (float32 X [n, 3], winding [n], sdf [n]); 0 or None = that
        output is not wanted, one of the two has to be.  Runs on the renderer's stream and, without
        stats, returns without waiting."""
        vp = [ctypes.c_void_p(p) if p else None for p in (x_ptr, winding_ptr, sdf_ptr)]
        st = NRStats()
        self._chk(self._L.nr_mesh_winding(self._m, vp[0], int(n), float(beta), vp[1], vp[2],
                                          NR_TRIMESH_BRUTE if brute else 0, NR_DEVICE,
                                          ctypes.byref(st) if with_stats else None))
        return st.as_dict() if with_stats else None

    # -- fitting samples (nr_mesh_sample, nr_mesh_fit_samples)
    def sample(self, n_surface, n_volume, seed=0, sigma=0.0, lo=-1.0, hi=1.0, tri=True, bary=True, with_stats=False):
        """nr_mesh_sample into host arrays: {"points" [n, 3][, "tri" [n] int32, "bary" [n, 3]]} -- n_surface
        points on the surface in proportion to triangle area (jittered by sigma times a unit-variance
        eight-term uniform sum), then n_volume points uniform in the box [lo, hi]; tri = -1 and bary = 0
        for those.  The bits are a function of the seed alone."""
        n = int(n_surface) + int(n_volume)
        out = {"points": np.zeros((max(n, 0), 3), np.float32)}
        if tri:
            out["tri"] = np.zeros(max(n, 0), np.int32)
        if bary:
            out["bary"] = np.zeros((max(n, 0), 3), np.float32)
        opts = _sample_opts(seed, n_surface, n_volume, sigma, lo, hi)
        st = NRStats()
        self._chk(self._L.nr_mesh_sample(self._m, ctypes.byref(opts), out["points"].ctypes.data,
                                         out["tri"].ctypes.data if tri else None, out["bary"].ctypes.data if bary else None,
                                         NR_HOST, ctypes.byref(st) if with_stats else None))
        return (out, st.as_dict()) if with_stats else out

    def sample_device(self, points_ptr, n_surface, n_volume, seed=0, sigma=0.0, lo=-1.0, hi=1.0, tri_ptr=None, bary_ptr=None,
                      with_stats=False):
        """nr_mesh_sample into device buffers (float32 points [n, 3], int32 tri [n], float32 bary [n, 3]); runs
        on the renderer's stream and, without stats, returns without waiting."""
        opts = _sample_opts(seed, n_surface, n_volume, sigma, lo, hi)
        vp = [ctypes.c_void_p(p) if p else None for p in (points_ptr, tri_ptr, bary_ptr)]
        st = NRStats()
        self._chk(self._L.nr_mesh_sample(self._m, ctypes.byref(opts), *vp, NR_DEVICE, ctypes.byref(st) if with_stats else None))
        return st.as_dict() if with_stats else None

    def fit_samples(self, n_surface, n_volume, seed=0, sigma=0.0, lo=-1.0, hi=1.0, sign="normal", beta=0.0, with_stats=False):
        """nr_mesh_fit_samples into host arrays: (X [n, 3], Y [n]) -- the samples of sample(), shuffled, with
        their signed distances (sign "normal": distance(); "winding": winding(sdf=True))."""
        n = int(n_surface) + int(n_volume)
        X, Y = np.zeros((max(n, 0), 3), np.float32), np.zeros(max(n, 0), np.float32)
        opts = _sample_opts(seed, n_surface, n_volume, sigma, lo, hi, sign, beta)
        st = NRStats()
        self._chk(self._L.nr_mesh_fit_samples(self._m, ctypes.byref(opts), X.ctypes.data, Y.ctypes.data, NR_HOST,
                                              ctypes.byref(st) if with_stats else None))
        return (X, Y, st.as_dict()) if with_stats else (X, Y)

    def fit_samples_device(self, x_ptr, y_ptr, n_surface, n_volume, seed=0, sigma=0.0, lo=-1.0, hi=1.0, sign="normal", beta=0.0,
                           with_stats=False):
        """nr_mesh_fit_samples into device buffers (float32 X [n, 3], Y [n]), ready for Fit.run_device; runs on
        the renderer's stream and, without stats, returns without waiting."""
        opts = _sample_opts(seed, n_surface, n_volume, sigma, lo, hi, sign, beta)
        st = NRStats()
        self._chk(self._L.nr_mesh_fit_samples(self._m, ctypes.byref(opts), ctypes.c_void_p(x_ptr), ctypes.c_void_p(y_ptr),
                                              NR_DEVICE, ctypes.byref(st) if with_stats else None))
        return st.as_dict() if with_stats else None

    # -- the signed distance on a lattice, remeshed (nr_mesh_sample_grid, nr_mesh_remesh, nr_mesh_remesh_sparse)
    @staticmethod
    def _sign(sign):
        return NR_SAMPLE_SIGN[sign] if isinstance(sign, str) else int(sign)

    def sample_grid(self, origin, step, dims, sign="normal", beta=0.0, brute=False, with_stats=False):
        """nr_mesh_sample_grid: the mesh's signed distance at the lattice points origin + (i, j, k) *
        step, dims = (nx, ny, nz), generated in the kernel -- bit for bit distance() (sign "normal") or
        winding(sdf=True) (sign "winding", with beta) of those points.  Returns float32 [nz, ny, nx]."""
        o, s, d = _lattice(origin, step, dims)
        out = np.zeros((d[2], d[1], d[0]), np.float32)
        st = NRStats()
        self._chk(self._L.nr_mesh_sample_grid(self._m, _fptr(o), _fptr(s), d, self._sign(sign), float(beta),
                                                 NR_TRIMESH_BRUTE if brute else 0, out.ctypes.data, NR_HOST,
                                                 ctypes.byref(st) if with_stats else None))
        return (out, st.as_dict()) if with_stats else out

    def sample_grid_device(self, sdf_ptr, origin, step, dims, sign="normal", beta=0.0, brute=False, with_stats=False):
        """nr_mesh_sample_grid into a device buffer of nx * ny * nz float32.  Runs on the renderer's
        stream and, without stats, returns without waiting."""
        o, s, d = _lattice(origin, step, dims)
        st = NRStats()
        self._chk(self._L.nr_mesh_sample_grid(self._m, _fptr(o), _fptr(s), d, self._sign(sign), float(beta),
                                                 NR_TRIMESH_BRUTE if brute else 0, ctypes.c_void_p(sdf_ptr), NR_DEVICE,
                                                 ctypes.byref(st) if with_stats else None))
        return st.as_dict() if with_stats else None

    def remesh(self, origin, step, dims, iso=0.0, sign="normal", beta=0.0, source_tri=True, with_stats=False):
        """nr_mesh_remesh: sample the lattice on the device and mesh it, as Renderer.extract_mesh.
        Returns a dict with "vertices" [nv, 3] float32, "triangles" [nt, 3] int32 and, with
        source_tri=True, "source_tri" [nv] int32 (the original triangle nearest each vertex).  With sign
        "winding" an open or self-overlapping mesh comes back closed and consistently oriented.  The
        count-only call comes first (it samples the lattice too), then the buffers are allocated."""
        o, s, d = _lattice(origin, step, dims)
        nv, nt = ctypes.c_long(0), ctypes.c_long(0)
        st = NRStats()

        def call(V, S, T):
            return self._L.nr_mesh_remesh(self._m, _fptr(o), _fptr(s), d, float(iso), self._sign(sign), float(beta),
                                             None if V is None else V.ctypes.data, None if S is None else S.ctypes.data,
                                             0 if V is None else V.shape[0], None if T is None else T.ctypes.data,
                                             0 if T is None else T.shape[0], ctypes.byref(nv), ctypes.byref(nt), NR_HOST,
                                             ctypes.byref(st) if with_stats else None)

        self._chk(call(None, None, None))
        V, T = np.zeros((nv.value, 3), np.float32), np.zeros((nt.value, 3), np.int32)
        S = np.zeros((nv.value,), np.int32) if source_tri else None
        if nv.value:
            self._chk(call(V, S, T))
        out = {"vertices": V, "triangles": T}
        if source_tri:
            out["source_tri"] = S
        return (out, st.as_dict()) if with_stats else out

    def remesh_device(self, origin, step, dims, vertices_ptr, v_cap, triangles_ptr, t_cap, iso=0.0, sign="normal", beta=0.0,
                      source_tri_ptr=None, with_stats=False):
        """nr_mesh_remesh into device buffers (v_cap x 3 float32 vertices, v_cap int32 source_tri, t_cap x
        3 int32 triangles; both vertices_ptr and triangles_ptr None: count only), on the renderer's
        stream.  Returns (nv, nt), with the stats dict appended with_stats=True; short capacities raise
        NRError with nothing written."""
        o, s, d = _lattice(origin, step, dims)
        vp = [ctypes.c_void_p(p) if p else None for p in (vertices_ptr, source_tri_ptr, triangles_ptr)]
        nv, nt = ctypes.c_long(0), ctypes.c_long(0)
        st = NRStats()
        self._chk(self._L.nr_mesh_remesh(self._m, _fptr(o), _fptr(s), d, float(iso), self._sign(sign), float(beta), vp[0],
                                            vp[1], int(v_cap), vp[2], int(t_cap), ctypes.byref(nv), ctypes.byref(nt),
                                            NR_DEVICE, ctypes.byref(st) if with_stats else None))
        res = (nv.value, nt.value)
        return res + (st.as_dict(),) if with_stats else res

    def remesh_sparse(self, origin, step, dims, iso=0.0, sign="normal", beta=0.0, brick=8, band=None, source_tri=True,
                      keys=True, with_stats=False):
        """nr_mesh_remesh_sparse: remesh() restricted to the bricks of brick^3 cells that have a corner
        within `band` of iso (or a sign change, or a NaN), as Renderer.extract_mesh_sparse.  band=None is
        the brick's diagonal, which is sound for a distance field (brick >= 4); for the winding sign of an
        open mesh band=float("inf") is the safe choice.  Returns a dict with "vertices", "triangles",
        "active_bricks" and, as asked, "source_tri" [nv] int32 and "keys" [nv] int64 (np.argsort(keys) is
        the dense mesh's vertex order)."""
        o, s, d = _lattice(origin, step, dims)
        bandf = self.owner._sparse_band(s, brick, band)
        nv, nt, na = ctypes.c_long(0), ctypes.c_long(0), ctypes.c_long(0)
        st = NRStats()

        def call(V, S, K, T):
            return self._L.nr_mesh_remesh_sparse(
                self._m, _fptr(o), _fptr(s), d, float(iso), self._sign(sign), float(beta), int(brick), bandf,
                None if V is None else V.ctypes.data, None if S is None else S.ctypes.data,
                None if K is None else K.ctypes.data, 0 if V is None else V.shape[0],
                None if T is None else T.ctypes.data, 0 if T is None else T.shape[0],
                ctypes.byref(nv), ctypes.byref(nt), ctypes.byref(na), NR_HOST, ctypes.byref(st) if with_stats else None)

        self._chk(call(None, None, None, None))
        V, T = np.zeros((nv.value, 3), np.float32), np.zeros((nt.value, 3), np.int32)
        S = np.zeros((nv.value,), np.int32) if source_tri else None
        K = np.zeros((nv.value,), np.int64) if keys else None
        if nv.value:
            self._chk(call(V, S, K, T))
        out = {"vertices": V, "triangles": T, "active_bricks": na.value}
        if source_tri:
            out["source_tri"] = S
        if keys:
            out["keys"] = K
        return (out, st.as_dict()) if with_stats else out

    def remesh_sparse_device(self, origin, step, dims, vertices_ptr, v_cap, triangles_ptr, t_cap, iso=0.0, sign="normal",
                             beta=0.0, brick=8, band=None, source_tri_ptr=None, keys_ptr=None, with_stats=False):
        """nr_mesh_remesh_sparse into device buffers (as remesh_device, and v_cap int64 keys), on the
        renderer's stream.  Returns (nv, nt, active_bricks), with the stats dict appended with_stats=True."""
        o, s, d = _lattice(origin, step, dims)
        vp = [ctypes.c_void_p(p) if p else None for p in (vertices_ptr, source_tri_ptr, keys_ptr, triangles_ptr)]
        nv, nt, na = ctypes.c_long(0), ctypes.c_long(0), ctypes.c_long(0)
        st = NRStats()
        self._chk(self._L.nr_mesh_remesh_sparse(
            self._m, _fptr(o), _fptr(s), d, float(iso), self._sign(sign), float(beta), int(brick),
            self.owner._sparse_band(s, brick, band), vp[0], vp[1], vp[2], int(v_cap), vp[3], int(t_cap), ctypes.byref(nv),
            ctypes.byref(nt), ctypes.byref(na), NR_DEVICE, ctypes.byref(st) if with_stats else None))
        res = (nv.value, nt.value, na.value)
        return res + (st.as_dict(),) if with_stats else res

    # -- rays (nr_mesh_trace_rays, nr_mesh_gbuffer, nr_mesh_render)
    _RAY_KEYS =("status", "t", "tri", "bary", "position", "normal")

    @staticmethod
    def _ray_flags(smooth, any_hit, brute):
        return (NR_MESH_RAY_SMOOTH if smooth else 0) | (NR_MESH_RAY_ANY if any_hit else 0) | (NR_TRIMESH_BRUTE if brute else 0)

    @staticmethod
    def _ray_outputs(shape, tri, bary, position, normal, any_hit):
        out = {"status": np.zeros(shape, np.int32)}
        if not any_hit:
            out["t"] = np.zeros(shape, np.float32)
            if tri:
                out["tri"] = np.zeros(shape, np.int32)
            for key, want in (("bary", bary), ("position", position), ("normal", normal)):
                if want:
                    out[key] = np.zeros(shape + (3,), np.float32)
        return out

    def trace_rays(self, origins, dirs, tmin=0.0, tmax=float("inf"), tri=True, bary=False, position=True, normal=True,
                   smooth=False, any_hit=False, brute=False, with_stats=False):
        """nr_mesh_trace_rays on host arrays: the closest hit of each ray p = origins[i] + t * dirs[i]
        (dirs as given) with tmin <= t <= tmax, bit for bit the arithmetic of include/neural_render.h.
        Returns {"status" (NR_RAY_HIT / NR_RAY_MISS), "t"[, "tri", "bary" [n, 3], "position" [n, 3],
        "normal" [n, 3]]}; smooth: the normal interpolated from the vertex pseudonormals instead of
        the face's.  any_hit: {"status"} only -- is anything hit (shadow and occlusion rays).  brute:
        every triangle, no hierarchy (the same bits).  Neighbours in space should be neighbours in
        the arrays."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError(f"origins {o.shape} and dirs {d.shape} differ")
        n = o.shape[0]
        out = self._ray_outputs((n,), tri, bary, position, normal, any_hit)
        ptr = [out[k].ctypes.data if k in out else None for k in self._RAY_KEYS]
        st = NRStats()
        self._chk(self._L.nr_mesh_trace_rays(self._m, o.ctypes.data, d.ctypes.data, n, float(tmin), float(tmax), *ptr,
                                             self._ray_flags(smooth, any_hit, brute), NR_HOST,
                                             ctypes.byref(st) if with_stats else None))
        return (out, st.as_dict()) if with_stats else out

    def trace_rays_device(self, origins_ptr, dirs_ptr, n, tmin=0.0, tmax=float("inf"), status_ptr=None, t_ptr=None,
                          tri_ptr=None, bary_ptr=None, position_ptr=None, normal_ptr=None, smooth=False, any_hit=False,
                          brute=False, with_stats=False):
        """nr_mesh_trace_rays on device buffers (float32 [n, 3] rays, int32 status / tri, float32 t,
        [n, 3] bary / position / normal); None = that output is not wanted.  Runs on the renderer's
        stream and, without stats, returns without waiting."""
        vp = [ctypes.c_void_p(p) if p else None
              for p in (origins_ptr, dirs_ptr, status_ptr, t_ptr, tri_ptr, bary_ptr, position_ptr, normal_ptr)]
        st = NRStats()
        self._chk(self._L.nr_mesh_trace_rays(self._m, vp[0], vp[1], int(n), float(tmin), float(tmax), *vp[2:],
                                             self._ray_flags(smooth, any_hit, brute), NR_DEVICE,
                                             ctypes.byref(st) if with_stats else None))
        return st.as_dict() if with_stats else None

    def gbuffer(self, W, H, tri=True, bary=False, position=True, normal=True, smooth=False, any_hit=False, brute=False,
                with_stats=False):
        """nr_mesh_gbuffer: the trace_rays outputs for the W x H pixel rays of the renderer's view
        (Renderer.render's rays), shaped (H, W) and (H, W, 3)."""
        out = self._ray_outputs((H, W), tri, bary, position, normal, any_hit)
        ptr = [out[k].ctypes.data if k in out else None for k in self._RAY_KEYS]
        st = NRStats()
        self._chk(self._L.nr_mesh_gbuffer(self._m, int(W), int(H), *ptr, self._ray_flags(smooth, any_hit, brute), NR_HOST,
                                          ctypes.byref(st) if with_stats else None))
        return (out, st.as_dict()) if with_stats else out

    def gbuffer_device(self, W, H, status_ptr=None, t_ptr=None, tri_ptr=None, bary_ptr=None, position_ptr=None,
                       normal_ptr=None, smooth=False, any_hit=False, brute=False, with_stats=False):
        """nr_mesh_gbuffer into device buffers; None = that output is not wanted."""
        vp = [ctypes.c_void_p(p) if p else None for p in (status_ptr, t_ptr, tri_ptr, bary_ptr, position_ptr, normal_ptr)]
        st = NRStats()
        self._chk(self._L.nr_mesh_gbuffer(self._m, int(W), int(H), *vp, self._ray_flags(smooth, any_hit, brute), NR_DEVICE,
                                          ctypes.byref(st) if with_stats else None))
        return st.as_dict() if with_stats else None

    def render(self, W, H, smooth=False, brute=False, with_stats=True):
        """nr_mesh_render: the mesh through the renderer's view, coloured as Renderer.render colours
        its normals (set_color_type / set_matcap of the renderer); (img [H, W] uint32, stats)."""
        out = np.zeros((H, W), np.uint32)
        st = NRStats()
        self._chk(self._L.nr_mesh_render(self._m, out.ctypes.data, int(W), int(H), self._ray_flags(smooth, False, brute),
                                         NR_HOST, ctypes.byref(st) if with_stats else None))
        return (out, st.as_dict()) if with_stats else out

    def render_device(self, out_ptr, W, H, smooth=False, brute=False, with_stats=False):
        """nr_mesh_render into a device buffer (uint32 [H, W])."""
        st = NRStats()
        self._chk(self._L.nr_mesh_render(self._m, ctypes.c_void_p(out_ptr), int(W), int(H),
                                         self._ray_flags(smooth, False, brute), NR_DEVICE,
                                         ctypes.byref(st) if with_stats else None))
        return st.as_dict() if with_stats else None
