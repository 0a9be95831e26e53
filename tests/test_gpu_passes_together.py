"""The optional passes of a wavefront trace on one context against each pass alone, on the MI355X: AOVs (both targets), ID mattes (K = 4),
motion vectors and the variance AOV share one workspace, one set of cleared records and one launch sequence (csrc/wf_passes.hip), and
none may see another.  Every comparison is bit for bit: each target, the output and the ray counts by kind of the context with all passes
equal those of the context with that pass alone.  Camera frames plain and under adaptive sampling, a bake with uncovered texels, a probe
atlas with a cell without a probe; 2 samples per trace, three accumulating calls each."""
import numpy as np
import pytest

from tests import adaptive_ref as ar
from tests import matte_ref as mr
from tests import test_gpu_bake as tb
from tests import test_gpu_variance as tv
from tests.test_gpu_variance import bits, copy_settings, same

pytestmark = pytest.mark.gpu
W, H = 40, 24                      # 3 x 2 tiles, partial on both edges
SPP, CALLS = 2, 3
POISON = 7.0
CAMERA = ("aov", "matte", "motion", "variance")
ATLAS = ("aov", "matte", "variance")          # motion vectors describe camera rays
TARGETS = {"aov": ("albedo", "normal_depth"), "matte": ("matte0", "matte1"), "motion": ("motion",), "variance": ("variance",)}
COUNTS = ("rays", "rays_primary", "rays_bounce", "rays_shadow", "closest_hits", "texture_taps", "accumulated_frames")


def tile_box(y, x):
    return slice(16 * y, 16 * y + 16), slice(16 * x, 16 * x + 16)


def run(s, passes, size=(W, H), setup=None, adaptive=None):
    """CALLS accumulating calls of SPP samples with `passes` on: the output and the passes' targets by name, the ray counts and, under
    adaptive sampling, the tiles' sample counts after every call.  The tiles retired by the first call are poisoned in every image
    right after it, so that what a later call writes there shows."""
    from gltf_renderer_amd.renderer import Renderer
    r = Renderer(0)
    env = s.upload(r)["env"]
    w, h = size
    s.width, s.height = w, h
    img = {name: r.create_output(w, h) for p in passes for name in TARGETS[p]}
    img["output"] = r.create_output(w, h)
    for t in img.values():
        t.fill_(POISON)
    if setup is not None:
        setup(r)
    r.set_samples_per_trace(SPP)
    if adaptive is not None:
        r.set_adaptive(*adaptive)
    p0 = s.execute_params(0, env_handle=env)
    if "aov" in passes:
        r.set_aov(img["albedo"], img["normal_depth"])
    if "matte" in passes:
        r.set_matte(mr.INSTANCE, [img["matte0"], img["matte1"]])
    if "motion" in passes:
        r.set_motion(img["motion"], list(p0.world_to_view), list(p0.view_to_clip))
    if "variance" in passes:
        r.set_variance(img["variance"])
    st = copy_settings(s.settings); st.reset = 1
    r.reset_stats()
    samples, retired = [], []
    for k in range(CALLS):
        r.trace(st, s.execute_params(k * SPP, env_handle=env), img["output"]); st.reset = 0
        if adaptive is not None:
            _, count, error, _ = r.adaptive_read(w, h)
            samples.append(count.copy())
            if k == 0:          # the rule of pt_set_adaptive: min_samples reached (SPP, below the cap) and the error within the threshold
                retired = [t for t in np.ndindex(count.shape) if count[t] >= adaptive[0] and error[t] <= adaptive[2]]
                for t in img.values():
                    for (y, x) in retired:
                        t[tile_box(y, x)] = POISON
    q = r.stats()
    got = dict(images={n: r.readback(t) for n, t in img.items()}, counts={n: getattr(q, n) for n in COUNTS}, samples=samples, retired=retired)
    r.close()
    return got


def check_together_equals_alone(s, passes, **kw):
    """Returns the run with every pass on."""
    both = run(s, passes, **kw)
    assert both["counts"]["rays_primary"] > 0 and both["counts"]["accumulated_frames"] == SPP * CALLS
    assert both["counts"]["rays"] == both["counts"]["rays_primary"] + both["counts"]["rays_bounce"] + both["counts"]["rays_shadow"]
    for p in passes:
        alone = run(s, (p,), **kw)
        for name in TARGETS[p] + ("output",):
            a, b = both["images"][name], alone["images"][name]
            assert same(a, b), (p, name, int((bits(a) != bits(b)).any(axis=-1).sum()))
        assert both["counts"] == alone["counts"], p
        assert all(np.array_equal(a, b) for a, b in zip(both["samples"], alone["samples"])) and both["retired"] == alone["retired"], p
    for name, a in both["images"].items():
        assert not np.array_equal(a, np.full_like(a, POISON)), name            # every pass wrote its targets
    return both


def test_camera_frames():
    both = check_together_equals_alone(tv.main_scene(), CAMERA)
    assert not any((a == POISON).all(axis=-1).any() for a in both["images"].values())          # every pixel of every image, partial tiles too
    assert both["images"]["variance"][..., 3].max() > 0 and both["images"]["albedo"][..., 3].max() == 1


def test_camera_frames_under_adaptive_sampling():
    """The tiles that see only the constant environment colour have error 0 and retire with the first call, at min_samples = SPP; the
    others never meet a threshold of 0 and take every call."""
    both = check_together_equals_alone(tv.sky_scene(), CAMERA, adaptive=(SPP, SPP * CALLS, 0.0))
    before_last, final = both["samples"][CALLS - 2], both["samples"][CALLS - 1]
    print("tile samples", final.tolist())
    assert (before_last == SPP).any(), before_last                                      # a tile retired before the last call ...
    assert (final == SPP * CALLS).any(), final                                           # ... and one that did not
    assert both["retired"] and all(final[t] == SPP for t in both["retired"])
    for name, a in both["images"].items():
        for (y, x) in both["retired"]:
            assert np.all(ar.tile_view(a, y, x) == POISON), (name, y, x)                 # a retired tile is unwritten in every target
        for (y, x) in np.ndindex(final.shape):
            if final[y, x] == SPP * CALLS:
                assert not np.any((ar.tile_view(a, y, x) == POISON).all(axis=-1)), (name, y, x)


def test_a_bake_with_uncovered_texels():
    """The quad's chart is the top left 0.6 x 0.6 of the 40 x 24 atlas: columns 24 .. 39 and rows 15 .. 23 hold no covered texel, and
    the generate stage writes their records."""
    s = tb.lit_scene(chart=0.6)
    both = check_together_equals_alone(s, ATLAS, setup=lambda r: r.set_bake(tb.OFFSET, 0, 0))
    out, alb, nd = (both["images"][n] for n in ("output", "albedo", "normal_depth"))
    uncovered = (bits(alb) == 0).all(axis=-1)
    assert uncovered[:, 25:].all() and uncovered[16:].all() and not uncovered[:14, :23].any()
    assert same(out[uncovered], np.broadcast_to(np.array([0, 0, 0, 1], np.float32), out[uncovered].shape)) and (bits(nd[uncovered]) == 0).all()
    assert (bits(both["images"]["variance"][uncovered]) == 0).all()


def test_a_probe_atlas_with_a_cell_without_a_probe():
    s = tv.main_scene()
    size = {}

    def setup(r):
        size["atlas"] = r.set_probes([(0.0, -0.5, 1.2), (0.6, -0.4, 1.0), (-0.5, -0.3, 0.9)], 16, columns=2)

    both = check_together_equals_alone(s, ATLAS, size=(32, 32), setup=setup)
    assert size["atlas"] == (32, 32)
    empty = np.s_[16:, 16:]                                                              # cell (1, 1): probe 3 of 3 does not exist
    out = both["images"]["output"]
    assert same(out[empty], np.broadcast_to(np.array([0, 0, 0, 1], np.float32), out[empty].shape))
    for name in ("albedo", "normal_depth", "variance"):
        assert (bits(both["images"][name][empty]) == 0).all(), name
    assert both["images"]["albedo"][:16, :16, 3].max() == 1


def test_motion_vectors_under_a_bake_are_still_refused():
    from gltf_renderer_amd.renderer import MiptError, Renderer
    s = tb.lit_scene(chart=0.6)
    s.width, s.height = W, H
    r = Renderer(0)
    s.upload(r)
    out, target = r.create_output(W, H), r.create_output(W, H)
    out.fill_(POISON); target.fill_(POISON)
    r.set_bake(tb.OFFSET, 0, 0)
    p = s.execute_params(0)
    r.set_motion(target, list(p.world_to_view), list(p.view_to_clip))
    with pytest.raises(MiptError, match="motion vectors describe camera rays: not under a bake or probes"):
        r.trace(copy_settings(s.settings), p, out)
    assert np.all(r.readback(out) == POISON) and np.all(r.readback(target) == POISON)
    r.close()
