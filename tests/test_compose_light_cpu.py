"""nr_compose_render_lit without a GPU: tests/compose_light_ref.py (the numpy restatement of its
contract) pinned to compose_ref.trace, query_ref.facing and light_ref.ambient_occlusion, the inputs of
tests/compose_light_cases.py shown to exercise every rule, and what the library and the binding
promise before any launch."""
import ctypes
import inspect

import numpy as np

import compose_light_ref
import compose_ref
import cudaneuralrender_amd as nr
import light_ref
import query_ref
from compose_light_cases import LIGHT, LIGHT_DIR, SCENES, bound, network, reference
from query_ref import ESCAPED, HIT, LIMIT, MISS

F = np.float32


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def cross_part(r):
    """Pixels whose light was blocked by a part other than the one they lie on."""
    return int(((r["occluder"] >= 0) & (r["occluder"] != r["part"])).sum())


def scene_args(scene):
    names, parts, iv, steps, frame, ld = SCENES[scene]
    c, r = bound(scene)
    return [network(g)[3] for g in names], parts, c, r, iv, steps, frame, ld


def test_inputs_are_not_vacuous():
    # L3 at 96 x 96: 1,275 HIT pixels owned 659 / 452 / 164, 7,827 ESCAPED, 114 LIMIT; 734 shadow rays
    # (567 ESCAPED, 163 HIT, 4 LIMIT), 126 of the HIT ones blocked by another part than the pixel's; 404
    # penumbra values, 163 fully lit pixels, 889 ao < 1, no NaN normal
    r = reference("l3", 96, 96)
    g = r["gbuffer"]
    hit = g["status"] == HIT
    own = [int((g["part"][hit] == j).sum()) for j in range(3)]
    assert all(v >= 100 for v in own), own
    assert cross_part(r) >= 100
    sh = r["shadow"].reshape(-1)[hit]
    assert int(((sh > 0) & (sh < 1)).sum()) >= 300
    assert int((sh == 1).sum()) >= 100
    assert int((r["ao"] < 1).sum()) >= 500
    assert int((r["ray_status"] == LIMIT).sum()) >= 1
    assert int((r["ray_status"] == HIT).sum()) >= 100 and int((r["ray_status"] == ESCAPED).sum()) >= 300
    assert not np.isnan(g["normal"]).any()
    # every occluder is a part, and only pixels whose ray ended HIT have one
    ended_hit = np.zeros(96 * 96, bool)
    ended_hit[r["ray_pix"][r["ray_status"] == HIT]] = True
    assert np.array_equal(r["occluder"].reshape(-1) >= 0, ended_hit) and r["occluder"].max() <= 2
    # the ragged variant, with the cut: 230 hits, 118 shadow rays, 17 cross-part blocks
    s = reference("l3", 45, 37)
    assert cross_part(s) >= 10 and int((s["gbuffer"]["status"] == HIT).sum()) >= 200
    # eight shadow steps: most rays run out of iterations
    assert int((reference("l3", 96, 96, 8)["ray_status"] == LIMIT).sum()) >= 500
    # the other scenes: every part of `four` owns pixels, the 4-input scene has cross-part blocks
    f = reference("four", 48, 48)
    fh = f["gbuffer"]["status"] == HIT
    assert all(int((f["gbuffer"]["part"][fh] == j).sum()) >= 5 for j in range(4)) and cross_part(f) >= 10
    assert cross_part(reference("f4", 48, 48)) >= 10


def test_hard_shadows_are_zero_or_one():
    r = reference("l3", 45, 37, shadow_k=0.0)
    sh = r["shadow"]
    assert np.isin(bits(sh), bits(np.array([0.0, 1.0], F))).all()
    hit = r["gbuffer"]["status"].reshape(37, 45) == HIT
    assert int((sh[hit] == 0).sum()) >= 50 and int((sh[hit] == 1).sum()) >= 20


def test_light_off_is_the_facing_frame():
    nets, parts, c, rad, iv, steps, frame, ld = scene_args("l3")
    W, H = 45, 37
    r = compose_light_ref.render(nets, parts, c, rad, W, H, iv, steps, ld, frame=frame, **light_ref.LIGHT_OFF)
    O, D = query_ref.pixel_rays(W, H, iv)
    g, _ = compose_ref.trace(nets, parts, c, rad, O, D, steps, frame)
    want = query_ref.facing(g["normal"], D, g["status"]).reshape(H, W)
    assert (want != 0).sum() >= 200 and len(np.unique(want)) >= 20
    assert np.array_equal(r["out"], want)
    assert np.array_equal(bits(r["ao"]), bits(np.ones((H, W), F))) and np.array_equal(bits(r["shadow"]), bits(np.ones((H, W), F)))
    assert (r["occluder"] == -1).all() and len(r["ray_pix"]) == 0


def test_shadow_march_is_the_composed_tracer():
    nets, parts, c, rad, iv, steps, frame, ld = scene_args("l3")
    r = reference("l3", 45, 37)
    g = r["gbuffer"]
    pix = r["ray_pix"]
    o = (g["position"][pix] + g["normal"][pix] * F(LIGHT["shadow_bias"])).astype(F)
    for shadow_steps in (64, 8):
        sh, status, nsteps, occ, pairs = compose_light_ref.shadow_march(nets, parts, c, rad, o, ld, shadow_steps, 0.0, frame)
        t, tst = compose_ref.trace(nets, parts, c, rad, o, np.broadcast_to(np.asarray(ld, F), o.shape), shadow_steps, frame,
                                   normals=False)
        assert np.array_equal(status, t["status"]) and np.array_equal(nsteps, t["steps"])
        assert np.array_equal(occ, t["part"]) and pairs == tst["part_evals"]
        assert np.array_equal(sh, np.where((status == HIT) | (status == LIMIT), F(0), F(1)))
    assert len(pix) >= 100 and MISS not in status


def test_lone_identity_part_occlusion_is_the_single_network_rule():
    nets, parts, c, rad, iv, steps, frame, ld = scene_args("one")
    assert bits(c).tolist() == [0, 0, 0] and float(rad) == float(F(1.2))
    r = reference("one", 48, 48)
    g = r["gbuffer"]
    hit = np.flatnonzero(g["status"] == HIT)
    assert hit.size >= 200
    want = light_ref.ambient_occlusion(nets[0], g["position"][hit], g["normal"][hit], LIGHT["ao_step"], LIGHT["ao_strength"],
                                       scene=nr.NR_SCENE["tanh"], frame=frame)
    got = r["ao"].reshape(-1)[hit]
    assert np.array_equal(bits(got), bits(want))
    assert int((got < 1).sum()) >= 100


def test_library_and_binding_before_any_launch():
    """Fails on a library without the call."""
    L = nr.lib()
    assert hasattr(L, "nr_compose_render_lit") and "nr_compose_render_lit" in nr._lib.EXPORTS
    lt = nr.Renderer._light(LIGHT_DIR, 64, **LIGHT)
    buf = np.zeros(16, np.uint32)
    # a NULL composition is an error, not a crash, whatever else is given
    assert L.nr_compose_render_lit(None, buf.ctypes.data, 4, 4, 10, ctypes.byref(lt), None, None, None, None, 0, None) == -1
    assert b"nr_compose_render_lit" in L.nr_last_error(None)
    assert L.nr_compose_render_lit(None, None, 4, 4, 10, None, None, None, None, None, 0, None) == -1
    assert L.nr_abi_version() == 3
    for name in ("render_lit", "render_lit_device"):
        sig = inspect.signature(getattr(nr.Composition, name))
        want = dict(shadow_steps=64, shadow_bias=0.01, shadow_k=8.0, ao_step=0.02, ao_strength=2.0, ambient=0.3, max_steps=6000,
                    with_stats=False)
        assert {k: sig.parameters[k].default for k in want} == want, name
    sig = inspect.signature(nr.Composition.render_lit)
    assert [sig.parameters[k].default for k in ("buffers", "with_part", "with_occluder")] == [False, False, False]
    # the light's direction is three numbers, checked before the library is called
    comp = object.__new__(nr.Composition)
    comp._c = ctypes.c_void_p()
    try:
        comp.render_lit(4, 4, (1.0, 0.0))
    except ValueError:
        pass
    else:
        raise AssertionError("a two-component light direction was accepted")
