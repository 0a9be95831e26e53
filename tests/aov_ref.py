"""numpy float32 restatement of the first-hit AOVs (include/mipt.h pt_set_aov), used by tests/test_gpu_aov.py and checked on its own by
tests/test_aov_host.py.

  hit_mask        which pixels of a HIT_KIND debug frame are hits, given an environment colour no debug colour takes
  albedo_record   one sample of the albedo target from a COLOR debug frame: (rgb, 1) where hit, zeros where miss
  sanitize        a record with a non-finite component contributes zeros (all four components of that target)
  blend4          pt_vertex.h blend_sample's weight 1 / (n + 1) on all four components, through adaptive_ref.blend
  fold            the running mean after 1, 2, ... samples, blended in sample order
  encode_normal   (n + 1) / 2 in float32: what PT_DEBUG_OUTPUT_SHADING_NORMAL shows of the normal_depth target's xyz
  decode_normal   2 c - 1 in float32
"""
import numpy as np

from tests import adaptive_ref as ar

f32 = np.float32
FRONT, BACK = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)          # PT_DEBUG_OUTPUT_HIT_KIND


def hit_mask(hit_kind, env_color):
    """(H, W) bool from a HIT_KIND frame traced without accumulation and without an environment map; every pixel must be exactly the
    front colour, the back colour or the environment colour."""
    rgb = np.asarray(hit_kind, f32)[..., :3]
    front = np.all(rgb == np.array(FRONT, f32), axis=-1)
    back = np.all(rgb == np.array(BACK, f32), axis=-1)
    miss = np.all(rgb == np.array(env_color, f32), axis=-1)
    assert np.all(front | back | miss), "a HIT_KIND pixel that is neither hit nor miss"
    assert not np.any((front | back) & miss)
    return front | back


def sanitize(rec):
    rec = np.asarray(rec, f32)
    bad = ~np.all(np.isfinite(rec), axis=-1)
    out = rec.copy()
    out[bad] = 0
    return out


def albedo_record(color, mask):
    rec = np.zeros(np.asarray(color).shape[:-1] + (4,), f32)
    rec[..., :3] = np.where(mask[..., None], np.asarray(color, f32)[..., :3], f32(0))
    rec[..., 3] = mask.astype(f32)
    return sanitize(rec)


def blend4(h, n, v):
    """h with n samples in it, v the next one: h + (1 / (n + 1)) * (v - h) on every component."""
    h, v = np.asarray(h, f32), np.asarray(v, f32)
    out = ar.blend(h, n, v[..., :3])
    w = np.repeat(h[..., 3:4], 4, axis=-1)
    out[..., 3] = ar.blend(w, n, np.repeat(v[..., 3:4], 3, axis=-1))[..., 0]
    return out


def fold(records):
    """records[k] = the (..., 4) sample of frame k.  Returns the list of running means: entry n - 1 after n samples."""
    out, cur = [], None
    for n, r in enumerate(records):
        r = np.asarray(r, f32)
        cur = r.copy() if n == 0 else blend4(cur, n, r)
        out.append(cur.copy())
    return out


def encode_normal(xyz):
    return ((np.asarray(xyz, f32) + f32(1)) / f32(2)).astype(f32)


def decode_normal(c):
    return (f32(2) * np.asarray(c, f32) - f32(1)).astype(f32)
