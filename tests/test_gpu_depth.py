"""The fused kernels at every network depth, not only the bundled 7 hidden layers.

With 7 hidden 32x32 layers the kernels take their unrolled and streamed instances; every other depth
0..16 takes the run-time-depth instances, which have their own loops, pack offsets (pk_final,
lp32_final, x3_final) and register allocation.  tests/depth_nets.py supplies a dense random network
per depth whose zero set the tracers hit; everything here is BIT-EXACT against the CPU oracle's
restatements (precision 0 fp32, 1 bf16, 2 fp16, 4 fp32x3 over the library's own pack), which
tests/test_depth_cpu.py checks against fp64 at the same depths.  A network whose fp32x3 pack
nr_pack_x3 refuses (dense networks past ~8 hidden layers) runs fp32 where it would have run the
split: fp32x3 = the fp32 MLP, 16-bit frames with fp32 normals and no endgame.  17 hidden layers is
not a fused shape: the layered fallback renders it in fp32 and the fused-only calls refuse it.
The oracle's result is computed once per network and form and shared."""
import functools

import numpy as np
import pytest

import cudaneuralrender_amd as nr
import depth_nets
import grad_ref
import mesh_ref
import oracle
import query_ref

pytestmark = pytest.mark.gpu

DEPTHS = [0, 1, 2, 3, 6, 8, 15, 16]
PRECS = ["fp32", "bf16", "fp16", "fp32x3"]
OPREC = {"fp32": 0, "bf16": 1, "fp16": 2, "fp32x3": 4}
NPTS = 1500  # 5 full 256-point workgroups of the fp32 forms and a ragged tail of 220
RAGGED = [1, 17, 33, 49, 64, 65, 127, 129]
BOUND_BREAKER = {"fp32": 1500.0, "bf16": 3e6, "fp16": 1500.0, "fp32x3": 5.0}
W, H, STEPS, FRAME = depth_nets.FRAME_W, depth_nets.FRAME_H, depth_nets.FRAME_STEPS, depth_nets.FRAME
FRAME_NETS = [(0, 3), (1, 4), (3, 3), (8, 4), (16, 3)]  # (hidden layers, inputs)
FORMS = ["fp32", "bf16-pure", "fp16-pure", "bf16-endgame", "fp16-endgame", "fp32x3"]
QUERY_NETS = [(0, 3), (3, 4), (16, 3)]
GRAD_NETS = [(0, 3), (2, 4), (4, 3), (6, 4)]
REFUSED = (12, 4)  # a network whose fp32x3 pack is refused (tests/test_depth_cpu.py)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def net_lists(nh, in0):
    dims, K, B = depth_nets.cached_net(nh, in0)
    return list(dims), list(K), list(B)


@functools.lru_cache(maxsize=None)
def onet(nh, in0):
    """(OracleNet, ok): with the library's fp32x3 pack when nr_pack_x3 accepts the network (the
    16-bit tracers' normals and endgame then run the split), without it when it is refused."""
    dims, K, B = net_lists(nh, in0)
    a, f, ok = nr.pack_x3(dims, K, B)
    return oracle.OracleNet(K, B, x3_pack=(a, f) if ok else None), bool(ok)


@functools.lru_cache(maxsize=None)
def points(in0):
    X = depth_nets.cloud(in0, n=NPTS, seed=17, frames=(0, 3, 359))
    X.setflags(write=False)
    return X


def oracle_forward(nh, in0, prec, X):
    """What nr_mlp_forward computes in `prec`: fp32x3 of a refused pack is the fp32 MLP."""
    net, ok = onet(nh, in0)
    p = OPREC[prec]
    y = net.forward(X, precision=0 if (p == 4 and not ok) else p)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def forward_ref(nh, in0, prec):
    return oracle_forward(nh, in0, prec, points(in0))


def renderer(nh, in0, prec):
    r = nr.Renderer(0)
    r.load_mlp(*net_lists(nh, in0)).set_precision(prec)
    return r


# ---- nr_mlp_forward ----------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("in0", [3, 4])
@pytest.mark.parametrize("nh", DEPTHS)
def test_mlp_forward_bitexact(nh, in0, prec):
    ref = forward_ref(nh, in0, prec)
    assert np.isfinite(ref).all() and np.abs(ref).max() > 0.2
    with renderer(nh, in0, prec) as r:
        y = r.mlp_forward(points(in0))
    bad = bits(y) != bits(ref)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[0], float(np.abs(y - ref).max()))
    if prec != "fp32":
        # not the fp32 path in disguise (a refused fp32x3 pack is exactly that)
        assert same(y, forward_ref(nh, in0, "fp32")) == (prec == "fp32x3" and not onet(nh, in0)[1])


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("in0", [3, 4])
@pytest.mark.parametrize("nh", [2, 8])
def test_mlp_forward_ragged_batches(nh, in0, prec):
    """1 to 4 tiles of the fp32 forms, the 64- and 128-point 16-bit forms and ragged ends: a point's
    value does not depend on the batch it is in."""
    ref = forward_ref(nh, in0, prec)
    X = points(in0)
    with renderer(nh, in0, prec) as r:
        for n in RAGGED:
            y = r.mlp_forward(X[:n])
            assert same(y, ref[:n]), (n, int((bits(y) != bits(ref[:n])).sum()))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("in0", [3, 4])
@pytest.mark.parametrize("nh", [2, 8])
def test_mlp_forward_unclamped_relu_forms(nh, in0, prec):
    """nr_set_debug bit 9: the add + max (fp32) and v_pk_max (bf16) ReLU forms on the scaled packs
    compute the same bits."""
    with renderer(nh, in0, prec) as r:
        y = r.set_debug(1 << 9).mlp_forward(points(in0))
    assert same(y, forward_ref(nh, in0, prec))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("in0", [3, 4])
@pytest.mark.parametrize("nh", [2, 8])
def test_mlp_forward_points_beyond_the_pack_bound(nh, in0, prec):
    """A few points with a coordinate beyond the pack's input bound (fp32 1024, bf16 2^20, fp32x3 4;
    fp16 has none) among ordinary ones: waves holding one take the unclamped forms (fp32x3: that
    point the fp32 MLP), and the batch still matches the oracle."""
    X = points(in0)[:640].copy()
    far = [5, 64, 127, 200, 333, 639]
    for i, k in enumerate(far):
        X[k, i % 3] = BOUND_BREAKER[prec] * (-1.0 if i & 1 else 1.0)
    ref = oracle_forward(nh, in0, prec, X)
    assert np.isfinite(ref).all()
    with renderer(nh, in0, prec) as r:
        y = r.mlp_forward(X)
    assert same(y, ref), int((bits(y) != bits(ref)).sum())
    if prec == "fp32x3":
        assert onet(nh, in0)[1]
        y32 = oracle_forward(nh, in0, "fp32", X)
        assert same(y[far], y32[far])
        rest = np.setdiff1d(np.arange(len(X)), far)
        assert not same(y[rest], y32[rest])


@pytest.mark.parametrize("in0", [3, 4])
@pytest.mark.parametrize("nh", range(7))
def test_identity_padding_fp32(nh, in0):
    """depth_net and its pad_to_seven (identity layers appended up to 7 hidden layers; exact on the
    oracle, tests/test_depth_cpu.py): the run-time-depth instance against the unrolled one."""
    dims, K, B = net_lists(nh, in0)
    X = points(in0)
    with nr.Renderer(0) as r:
        y = r.load_mlp(dims, K, B).set_precision("fp32").mlp_forward(X)
        yp = r.load_mlp(*depth_nets.pad_to_seven(K, B)).mlp_forward(X)
    assert same(y, yp), int((bits(y) != bits(yp)).sum())
    assert np.abs(y).max() > 0.2


# ---- frames ------------------------------------------------------------------

@pytest.fixture(scope="module")
def chrome():
    return nr.load_png(nr.matcap_path("Chrome"))


def form_settings(form, ok):
    """(precision, tau, oracle precision, oracle endgame) of a frame form for a network whose fp32x3
    pack is / is not accepted."""
    prec = form.split("-")[0]
    tau = nr.NR_ENDGAME_DEFAULT if form.endswith("endgame") else 0.0
    op = OPREC[prec]
    if not ok:
        op = 0 if op == 4 else op
        return prec, tau, op, 0.0
    return prec, tau, op, (tau if op in (1, 2) else 0.0)


@functools.lru_cache(maxsize=None)
def frame_ref(nh, in0, scene, form):
    net, ok = onet(nh, in0)
    _, _, op, otau = form_settings(form, ok)
    iv, nm = nr.camera(*depth_nets.CAMERA)
    img, st = net.render(W, H, iv, nm, frame=FRAME, color_type=1, num_inputs=in0, scene=nr.NR_SCENE[scene],
                         matcap=nr.load_png(nr.matcap_path("Chrome")), max_steps=STEPS, nthreads=16, precision=op,
                         endgame=otau)
    img.setflags(write=False)
    return img, st


def check_frame(img, st, ref, rst, what):
    assert np.array_equal(img, ref), (what, int((img != ref).sum()))
    for k in ("ray_steps", "rays_hit", "rays_shaded"):
        assert st[k] == rst[k], (what, k, st, rst)
    assert st["rays_shaded"] > 0
    for k in ("endgame_evals", "endgame_switches"):
        assert st[k] == rst.get(k, 0), (what, k, st, rst)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scene", ["tanh", "v1"])
@pytest.mark.parametrize("nh,in0", FRAME_NETS)
def test_frames_bitexact(chrome, nh, in0, scene, form):
    ok = onet(nh, in0)[1]
    prec, tau, _, otau = form_settings(form, ok)
    ref, rst = frame_ref(nh, in0, scene, form)
    assert (ref != 0).any() and rst["rays_shaded"] > 0
    iv, nm = nr.camera(*depth_nets.CAMERA)
    with renderer(nh, in0, prec) as r:
        r.set_endgame(tau).set_view(iv, nm, FRAME).set_static(nr.NR_COLOR_MATCAP, in0).set_scene(scene).set_matcap(chrome)
        img, st = r.render(W, H, STEPS)
        check_frame(img, st, ref, rst, "persistent")
        if form == "fp32":
            imgs, bst = r.render_batch(W, H, [(iv, nm, FRAME)] * 2, STEPS)
            assert all(np.array_equal(b, ref) for b in imgs)
            assert bst["ray_steps"] == 2 * rst["ray_steps"] and bst["rays_shaded"] == 2 * rst["rays_shaded"]
        r.set_schedule("wavefront")
        img, st = r.render(W, H, STEPS)
        check_frame(img, st, ref, rst, "wavefront")
    if otau > 0:
        assert st["endgame_switches"] > 0 and st["endgame_evals"] >= st["endgame_switches"]
    else:
        assert st["endgame_evals"] == 0 and st["endgame_switches"] == 0


def test_frame_forms_differ():
    """The forms compared above are different frames (no form is another in disguise), and the
    endgame ran wherever the pack is accepted."""
    for nh, in0 in FRAME_NETS:
        ok = onet(nh, in0)[1]
        assert ok == (nh <= 8)
        f = {form: frame_ref(nh, in0, "tanh", form) for form in FORMS}
        assert not np.array_equal(f["fp32"][0], f["bf16-pure"][0])
        assert not np.array_equal(f["bf16-pure"][0], f["fp16-pure"][0])
        if ok:
            assert not np.array_equal(f["bf16-pure"][0], f["bf16-endgame"][0])
            assert f["bf16-endgame"][1]["endgame_switches"] > 0 and f["fp16-endgame"][1]["endgame_switches"] > 0


# ---- queries and lattices (always fp32) ----------------------------------------

def query_rays(n=300):
    rng = np.random.default_rng(23)
    o = rng.uniform(-1.6, 1.6, (n, 3))
    d = rng.uniform(-0.5, 0.5, (n, 3)) - o
    d[::3] = rng.normal(size=d[::3].shape)
    d[1::2] *= 0.5
    return o.astype(np.float32), d.astype(np.float32)


def assert_query(got, ref):
    for k in ("status", "steps", "t", "position", "normal"):
        bad = bits(got[k]).reshape(bits(ref[k]).shape) != bits(ref[k])
        assert not bad.any(), f"{k}: {int(bad.sum())} of {bad.size} differ, first {np.argwhere(bad)[0]}"


@pytest.mark.parametrize("nh,in0", QUERY_NETS)
def test_trace_rays(nh, in0):
    o, d = query_rays()
    ref, rst = query_ref.trace(onet(nh, in0)[0], o, d, STEPS, scene=nr.NR_SCENE["v1"], frame=FRAME)
    assert (ref["status"] == query_ref.HIT).sum() >= 30
    with renderer(nh, in0, "fp32") as r:
        r.set_static(nr.NR_COLOR_FACING, in0).set_scene("v1").set_view(*nr.camera(*depth_nets.CAMERA), FRAME)
        out, st = r.trace_rays(o, d, STEPS, with_stats=True)
    assert_query(out, ref)
    for k in ("ray_steps", "shade_evals", "rays_hit", "rays_shaded"):
        assert st[k] == rst[k], (k, st, rst)


@pytest.mark.parametrize("nh,in0", QUERY_NETS)
def test_render_gbuffer(nh, in0):
    iv, nm = nr.camera(*depth_nets.CAMERA)
    o, d = query_ref.pixel_rays(40, 32, iv)
    ref, rst = query_ref.trace(onet(nh, in0)[0], o, d, STEPS, scene=nr.NR_SCENE["tanh"], frame=FRAME)
    assert (ref["status"] == query_ref.HIT).sum() >= 100
    with renderer(nh, in0, "fp32") as r:
        r.set_static(nr.NR_COLOR_FACING, in0).set_scene("tanh").set_view(iv, nm, FRAME)
        out, st = r.render_gbuffer(40, 32, STEPS, with_stats=True)
    assert out["status"].shape == (32, 40) and out["normal"].shape == (32, 40, 3)
    assert_query({k: v.reshape(ref[k].shape) for k, v in out.items()}, ref)
    assert st["ray_steps"] == rst["ray_steps"] and st["rays_shaded"] == rst["rays_shaded"]


@pytest.mark.parametrize("nh,in0", QUERY_NETS)
def test_sample_grid(nh, in0):
    origin, step, dims = (-0.9, -0.8, -0.7), (0.11, 0.2, 0.35), (17, 9, 5)
    ref = mesh_ref.sample(onet(nh, in0)[0], origin, step, dims, scene=nr.NR_SCENE["v1"], frame=FRAME)
    assert (ref > 0).any() and (ref < 0).any()
    with renderer(nh, in0, "fp32") as r:
        r.set_static(nr.NR_COLOR_FACING, in0).set_scene("v1").set_view(*nr.camera(*depth_nets.CAMERA), FRAME)
        v = r.sample_grid(origin, step, dims)
    assert same(v, ref), int((bits(v) != bits(ref)).sum())


@pytest.mark.parametrize("nh,in0", GRAD_NETS)
def test_mlp_gradient(nh, in0):
    dims, K, B = net_lists(nh, in0)
    X = points(in0)[:1000]
    value, grad, normal = grad_ref.gradient(K, B, X)
    assert same(value, forward_ref(nh, in0, "fp32")[:1000, 0])
    with renderer(nh, in0, "fp32") as r:
        out = r.mlp_gradient(X, value=True, grad=True, normal=True)
    for k, ref in (("value", value), ("grad", grad), ("normal", normal)):
        bad = bits(out[k]) != bits(ref)
        assert not bad.any(), f"{k}: {int(bad.sum())} of {bad.size} words differ, first at {np.argwhere(bad)[0]}"
    assert np.abs(grad).max() > 0.05


# ---- a refused fp32x3 pack ------------------------------------------------------

def test_refused_pack_runs_fp32(chrome):
    """A network whose fp32x3 pack nr_pack_x3 refuses: NR_PRECISION_FP32X3 is the fp32 MLP bit for
    bit; the bf16 tracer takes fp32 normals and, whatever the threshold, no endgame."""
    nh, in0 = REFUSED
    net, ok = onet(nh, in0)
    assert not ok and net.x3 is None
    X = points(in0)
    with renderer(nh, in0, "fp32x3") as r:
        assert same(r.mlp_forward(X), forward_ref(nh, in0, "fp32"))
    iv, nm = nr.camera(*depth_nets.CAMERA)
    ref, rst = net.render(W, H, iv, nm, frame=FRAME, color_type=1, num_inputs=in0, scene=nr.NR_SCENE["v1"], matcap=chrome,
                          max_steps=STEPS, nthreads=16, precision=1)
    assert rst["rays_shaded"] > 0
    with renderer(nh, in0, "bf16") as r:
        r.set_endgame(nr.NR_ENDGAME_DEFAULT)
        r.set_view(iv, nm, FRAME).set_static(nr.NR_COLOR_MATCAP, in0).set_scene("v1").set_matcap(chrome)
        for sched in ("persistent", "wavefront"):
            img, st = r.set_schedule(sched).render(W, H, STEPS)
            check_frame(img, st, ref, rst, sched)
            assert st["endgame_evals"] == 0 and st["endgame_switches"] == 0


# ---- 17 hidden layers: not a fused shape ------------------------------------------

@functools.lru_cache(maxsize=None)
def net17():
    dims, K, B = depth_nets.depth_net(depth_nets.MAX_HIDDEN + 1, 3)
    return dims, K, B, oracle.OracleNet(K, B)


@pytest.mark.parametrize("prec", PRECS)
def test_seventeen_hidden_layers_take_the_layered_fallback(chrome, prec):
    dims, K, B, net = net17()
    X = points(3)
    iv, nm = nr.camera(*depth_nets.CAMERA)
    with nr.Renderer(0) as r:
        r.load_mlp(dims, K, B).set_precision(prec)
        assert same(r.mlp_forward(X), net.forward(X))
        r.set_view(iv, nm, FRAME).set_static(nr.NR_COLOR_MATCAP, 3).set_scene("v1").set_matcap(chrome)
        img, st = r.render(W, H, STEPS)
    ref, rst = net.render(W, H, iv, nm, frame=FRAME, color_type=1, scene=nr.NR_SCENE["v1"], matcap=chrome,
                          max_steps=STEPS, nthreads=16)
    assert np.array_equal(img, ref), int((img != ref).sum())
    assert st["ray_steps"] == rst["ray_steps"] and st["rays_shaded"] == rst["rays_shaded"] > 0


def test_seventeen_hidden_layers_refused_by_the_fused_only_calls():
    dims, K, B, _ = net17()
    o, d = query_rays(8)
    with nr.Renderer(0) as r:
        r.load_mlp(dims, K, B).set_view(*nr.camera(*depth_nets.CAMERA), FRAME)
        for call in (lambda: r.trace_rays(o, d, 10), lambda: r.sample_grid((0, 0, 0), (0.1, 0.1, 0.1), (2, 2, 2)),
                     lambda: r.mlp_gradient(points(3)[:8])):
            with pytest.raises(nr.NRError) as e:
                call()
            assert e.value.code == -4  # NR_E_FORMAT
