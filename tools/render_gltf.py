#!/usr/bin/env python3
"""Render a .gltf / .glb file on an MI355X through the C-ABI only: loader (include/mipt_scene.h) -> path tracer (include/mipt.h).

  python tools/render_gltf.py scene.glb --env sky.hdr --spp 64 --size 1280 720 --out frame.png [--animation 0 --time 0.5]
  python tools/render_gltf.py scene.glb --spp 256 --adaptive 0.05 --min-spp 16 --sample-map samples.png

--adaptive THRESHOLD: tile-level adaptive sampling (pt_set_adaptive): a 16x16 tile stops at --spp samples, or earlier once it has
--min-spp and its error estimate is <= THRESHOLD; the samples used are printed against tiles x spp.  --sample-map writes the
per-tile counts as a grey PNG (white = --spp).

--aov PREFIX: first-hit AOVs (pt_set_aov), accumulated with the frame: PREFIX_albedo.png (the mean albedo of the samples that hit,
rgb / coverage, linear, 8 bit), PREFIX_normal.png ((n / |n| + 1) / 2 of the mean world-space shading normal where coverage > 0,
black elsewhere) and PREFIX_depth.npy (float32 H x W: the mean of the camera rays' hit distances, a miss counting 0).

--denoise [ITERATIONS]: the a-trous filter over the first-hit AOVs (pt_denoise, 5 passes unless given) on the accumulated frame before tone
mapping; turns the AOVs on, and keeps the noisy frame beside the output as <out>_noisy.png (<out> without its extension).

--checkpoint FILE: after the last sample the accumulation (the frame, the AOVs, the adaptive tile state) is written to FILE
(pt_accum_save).  --resume FILE: loads such a file (pt_accum_load) and continues from the frame number it holds; --spp is the TOTAL, so
`--spp 64 --checkpoint a.acc` today and `--spp 256 --resume a.acc` tomorrow give the 256-sample frame of one uninterrupted run.  The file
must fit the command line: the same --size, --aov / --denoise or neither, and the same --adaptive, --min-spp and --spp (an adaptive
accumulation carries its sample cap); the scene, camera and --batch are the caller's to repeat.

--aperture R: thin-lens depth of field (pt_set_lens) with aperture radius R in world units; --focus D gives the view-space depth of the plane
in focus, --focus-pixel X,Y focuses on what that image position sees (pt_lens_focus_at; pixel units, the default is the image centre);
--blades N (3..16) makes the aperture a regular polygon, --blade-rotation DEG turns it.  The lens is not part of a checkpoint: with
--resume, give the same --aperture / --focus / --focus-pixel / --blades / --blade-rotation as the run that wrote it, or the accumulation
continues with another lens (a --focus-pixel that now hits other geometry included).
  python tools/render_gltf.py scene.glb --spp 256 --aperture 0.05 --focus-pixel 640,400 --blades 6

--bake W H: texture-space baking (pt_set_bake): the frame is a W x H UV atlas instead of a camera image (--size is ignored): the radiance that
leaves each texel along its surface normal -- for a diffuse surface, the lightmap.  --bake-uv {0,1} picks the UV set that addresses the atlas
(glTF's TEXCOORD_1 is conventionally the lightmap set), --bake-instance N bakes one row of the instance table (default: every instance with
that UV set), --surface-offset D starts the rays D world units above the surface (default: 1e-4 of the scene's bounding diagonal) and
--dilate N fills N texels beyond the charts' borders from their covered neighbours after the last sample (pt_bake_dilate; after --denoise).
Composes with --aov (albedo.w is the coverage), --denoise, --adaptive and --checkpoint / --resume (the bake is not part of a checkpoint: repeat
the bake options).  An ambient-occlusion map is a bake with a white diffuse world under a white sky: see INTEGRATION.md.
  python tools/render_gltf.py scene.glb --bake 1024 1024 --bake-uv 1 --spp 256 --dilate 4 --out lightmap.exr

--probes "x,y,z;x,y,z;...": light-probe baking (pt_set_probes): the frame is an atlas of octahedral maps, one --probe-res N x N map (a multiple of
16, default 32) per world-space position, instead of a camera image (--size is ignored): the radiance that arrives at each position from every
direction; it goes to --out.  --probe-sh OUT.npy writes the nine spherical-harmonic coefficients per channel of every probe (pt_probe_project,
a float32 array [probes, 9, 3]); with --irradiance they are scaled so that their sum over Y_lm(n) is the irradiance on a surface with normal n
(INTEGRATION.md has the shader side).  Composes with --aov (normal_depth.w is the probe's distance map), --adaptive and --checkpoint /
--resume (the probes are not part of a checkpoint: repeat the probe options).  Not together with --bake or --aperture.
  python tools/render_gltf.py scene.glb --probes "0,0,1;2,0,1;4,0,1" --probe-res 64 --spp 256 --probe-sh probes.npy --irradiance --out probes.exr

--matte instance|material: ID mattes (pt_set_matte): per pixel a ranked list of (id, coverage) pairs in Cryptomatte's layout -- which object
(row of the instance table) or material each pixel sees, anti-aliased -- accumulated with the frame.  --matte-ranks K (2, 4, 6 or 8, default 6)
pairs per pixel; --matte-out PREFIX writes one uncompressed 32-bit float RGBA EXR per layer, PREFIX_00.exr ... (R, B = the ids' bits, G, A =
their coverages; ranks 2j and 2j + 1 in layer j), and PREFIX.json, the manifest {"instance_<i>" | "material_<i>": id as 8 hex digits}.
Composes with --aov, --adaptive, --bake and --probes; the layers are not part of a checkpoint, so not with --checkpoint / --resume here.
  python tools/render_gltf.py scene.glb --spp 64 --matte instance --matte-ranks 6 --matte-out crypto --out frame.png

--motion-out FILE --prev-time T: the motion-vector pass (pt_set_motion) of an animated scene: poses --animation at time T, takes the snapshot of
that pose (pt_motion_snapshot), poses --time and accumulates, beside the frame, per pixel (previous minus current screen position in pixels,
previous view depth, current view depth); FILE is an uncompressed 32-bit float RGBA EXR (or a float32 .npy, H x W x 4).  The camera stands still.
  python tools/render_gltf.py figure.glb --animation 0 --prev-time 0.46 --time 0.5 --spp 16 --motion-out motion.exr

--sequence T0:T1:FPS: renders the frames of --animation at T0, T0 + 1 / FPS, ... <= T1, --spp samples each, to <out>_0000.<ext>, <out>_0001.<ext>,
...; every frame after the first carries the motion vectors against the frame before it.  With --temporal each frame is denoised (pt_denoise,
--denoise ITERATIONS or 5) and then blended with the previous filtered frame read at its motion vector (pt_reproject): the flicker of a
low-sample sequence denoised frame by frame goes.  Camera renders only: not with --bake, --probes, --adaptive, --matte, --checkpoint, --resume.
  python tools/render_gltf.py figure.glb --animation 0 --sequence 0:2:24 --temporal --spp 16 --out shot.png

--motion-blur SHUTTER: a shutter-time blur of the finished frame along its motion vectors (pt_motion_blur; SHUTTER in (0, 2] is the open share
of the frame interval, 0.5 = a 180 degree shutter), applied after --denoise and --temporal and before tone mapping.  --blur-radius R caps the
half streak (1..64 px, default 32), --blur-taps N sets the taps along it (2..64, default 16).  It needs motion vectors: use it with --sequence,
or with --prev-time T on a single frame (--motion-out is then optional).  A reconstruction filter, not ray-traced motion blur (include/mipt.h).
  python tools/render_gltf.py figure.glb --animation 0 --sequence 0:2:24 --temporal --motion-blur 0.5 --spp 16 --out shot.png
  python tools/render_gltf.py figure.glb --animation 0 --prev-time 0.46 --time 0.5 --motion-blur 0.5 --spp 64 --out frame.png

--bloom [STRENGTH]: the reference's bloom (pt_bloom: a dual-filter blur over a mip pyramid, added to the frame STRENGTH times; 0.01 unless
given, the reference's default), applied last before tone mapping: after --denoise, --denoise-variance, --temporal and --motion-blur, in
--sequence mode to every frame.  --bloom-radius N sets the pyramid levels (0..8, default 4: each level doubles the reach), --bloom-threshold T
lets only what is brighter than T glow (default 0 = everything, as upstream).  Not with --bake or --probes: an atlas is not a picture.
  python tools/render_gltf.py lantern.glb --spp 256 --denoise --bloom 0.04 --bloom-radius 6 --out frame.png

--env-cubes PREFIX: with --env, the environment's two raster-pass cubes (pt_env_filter at the reference's values): the prefiltered GGX chain as
PREFIX_ggx_0.npy, PREFIX_ggx_1.npy, ... (level i holds roughness (i / (levels - 1))^2) and the diffuse irradiance cube as PREFIX_diffuse.npy,
each a float16 array [6, n, n, 4].  The render itself is unchanged: the path tracer does not read them.
  python tools/render_gltf.py scene.glb --env sky.hdr --env-cubes sky --out frame.png

--variance-out PREFIX: the variance pass (pt_set_variance), accumulated with the frame: PREFIX.exr (32-bit float RGBA; a name ending in .npy
gives an array) holds the variance of each pixel's mean, V / (n - 1): rgb per channel, a of the channel sum.  --noise-target X keeps tracing
batches of --batch samples until no tile's relative standard error (pt_noise_estimate, adaptive sampling's own normalisation) exceeds X, or
--spp is reached.  Either option prints the noise summary.  Composes with --adaptive (the tiles' own counts), --aov, --denoise, --bake,
--probes and --matte; the target is not part of a checkpoint, so not with --checkpoint / --resume, and not with --sequence.
  python tools/render_gltf.py scene.glb --spp 1024 --noise-target 0.02 --variance-out noise --out frame.png

--denoise-variance [ITERATIONS]: the a-trous filter steered by the variance pass (pt_denoise_variance, 5 passes unless given) on the
accumulated frame, where --denoise runs: before --dilate, --motion-blur and tone mapping; turns on the AOVs and the variance pass, uses the
tiles' own counts under --adaptive and the samples traced otherwise, and keeps the noisy frame as <out>_noisy.png.  It leaves a converged
frame alone, which --denoise blurs; below about 4 samples a pixel --denoise is the better tool.  Not together with --denoise, --sequence,
--checkpoint or --resume.
  python tools/render_gltf.py scene.glb --spp 256 --adaptive 0.05 --denoise-variance --out frame.png

Camera: an orbit camera fitted to the scene's bounds (the reference's default controller, CameraController.h:42-49);
settings: the application defaults (Main.cpp:462-474) with --bounces."""
import argparse
import json
import math
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def aov_images(albedo, normal_depth):
    """(albedo rgb8, normal rgb8, depth float32) from the two accumulated AOV targets (H, W, 4)."""
    cover = albedo[..., 3]
    hit = cover > 0
    alb = np.zeros(albedo.shape[:2] + (3,), np.float32)
    alb[hit] = albedo[..., :3][hit] / cover[hit][:, None]
    n = normal_depth[..., :3].astype(np.float64)
    ln = np.linalg.norm(n, axis=-1)
    ok = hit & (ln > 0)
    enc = np.zeros(n.shape, np.float64)
    enc[ok] = (n[ok] / ln[ok][:, None] + 1.0) / 2.0
    to8 = lambda x: (np.clip(x, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    return to8(alb), to8(enc), np.ascontiguousarray(normal_depth[..., 3], np.float32)


def noisy_path(out):
    """Where --denoise keeps the frame as it was before the filter."""
    return os.path.splitext(out)[0] + "_noisy.png"


def resume_mismatch(info, size, aov, adaptive, accum_flags):
    """Why a checkpoint (its abi.PtAccumInfo) does not fit the command line, or None.  adaptive = (min_samples, max_samples, threshold) as
    --min-spp / --spp / --adaptive give them, or None; accum_flags = (ACCUM_ALBEDO, ACCUM_NORMAL_DEPTH, ACCUM_ADAPTIVE)."""
    a_alb, a_nd, a_ad = accum_flags
    if (info.width, info.height) != tuple(size):
        return "it holds a %d x %d frame, --size is %d x %d" % (info.width, info.height, size[0], size[1])
    if (info.tile_rank, info.tile_rank_count) != (0, 1):
        return "it holds tile shard %d of %d, this tool renders whole frames" % (info.tile_rank, info.tile_rank_count)
    has_aov = bool(info.sections & (a_alb | a_nd))
    if has_aov != bool(aov):
        return "it holds AOVs, give --aov or --denoise" if has_aov else "it holds no AOVs, drop --aov / --denoise"
    if bool(info.sections & a_ad) != (adaptive is not None):
        return "it is an adaptive accumulation, give --adaptive" if info.sections & a_ad else "it is a uniform accumulation, drop --adaptive"
    if adaptive is not None:
        c = info.adaptive
        have = (c.min_samples, c.max_samples, np.float32(c.threshold))
        want = (adaptive[0], adaptive[1], np.float32(adaptive[2]))
        if have != want:
            return "it was rendered with --min-spp %d --spp %d --adaptive %.9g, not %d / %d / %.9g" % (have + want)
    return None


def sequence_frames(spec):
    """"T0:T1:FPS" -> the frame times T0 + i / FPS <= T1 (a tolerance of a millionth of a frame); ValueError for anything else."""
    parts = spec.split(":")
    if len(parts) != 3:
        raise ValueError(spec)
    t0, t1, fps = (float(v) for v in parts)
    if not (math.isfinite(t0) and math.isfinite(t1) and math.isfinite(fps)) or fps <= 0 or t1 < t0:
        raise ValueError(spec)
    n = int(math.floor((t1 - t0) * fps + 1e-6)) + 1
    return [t0 + i / fps for i in range(n)]


def numbered_path(out, i):
    stem, ext = os.path.splitext(out)
    return "%s_%04d%s" % (stem, i, ext)


def write_exr_rgba32f(path, rgba):
    """An uncompressed scanline OpenEXR file with the four FLOAT channels A, B, G, R of an (H, W, 4) float32 image, bit for bit: the ids of a
    matte layer are 32-bit patterns, which neither a half-float nor a tone-mapped file keeps."""
    a = np.ascontiguousarray(rgba, np.float32)
    h, w = a.shape[:2]

    def attr(name, kind, data):
        return name.encode() + b"\0" + kind.encode() + b"\0" + struct.pack("<i", len(data)) + data

    chlist = b"".join(c.encode() + b"\0" + struct.pack("<iBBBBii", 2, 0, 0, 0, 0, 1, 1) for c in "ABGR") + b"\0"      # pixel type 2 = FLOAT
    box = struct.pack("<iiii", 0, 0, w - 1, h - 1)
    head = (struct.pack("<ii", 20000630, 2) + attr("channels", "chlist", chlist) + attr("compression", "compression", b"\0") + attr("dataWindow", "box2i", box) +
            attr("displayWindow", "box2i", box) + attr("lineOrder", "lineOrder", b"\0") + attr("pixelAspectRatio", "float", struct.pack("<f", 1.0)) +
            attr("screenWindowCenter", "v2f", struct.pack("<ff", 0.0, 0.0)) + attr("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0")
    line = 8 + 16 * w
    first = len(head) + 8 * h
    with open(path, "wb") as f:
        f.write(head)
        f.write(struct.pack("<%dQ" % h, *[first + y * line for y in range(h)]))
        for y in range(h):
            f.write(struct.pack("<ii", y, 16 * w))
            for ch in (3, 2, 1, 0):                                          # a scanline holds its channels in alphabetical order
                f.write(a[y, :, ch].tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("path")
    ap.add_argument("--env", default="")
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--size", type=int, nargs=2, default=[1280, 720])
    ap.add_argument("--bounces", type=int, default=5)
    ap.add_argument("--animation", type=int, default=-1)
    ap.add_argument("--time", type=float, default=0.0)
    ap.add_argument("--azimuth", type=float, default=0.6)
    ap.add_argument("--inclination", type=float, default=-0.35)
    ap.add_argument("--out", default="frame.png")
    ap.add_argument("--adaptive", type=float, default=None, metavar="THRESHOLD")
    ap.add_argument("--min-spp", type=int, default=16)
    ap.add_argument("--batch", type=int, default=8, help="samples per pt_trace with --adaptive")
    ap.add_argument("--sample-map", default="")
    ap.add_argument("--aov", default="", metavar="PREFIX")
    ap.add_argument("--denoise", type=int, nargs="?", const=5, default=None, metavar="ITERATIONS")
    ap.add_argument("--denoise-variance", type=int, nargs="?", const=5, default=None, metavar="ITERATIONS",
                    help="the a-trous filter steered by the variance pass (pt_denoise_variance); not with --denoise, --sequence, --checkpoint, --resume")
    ap.add_argument("--checkpoint", default="", metavar="FILE", help="write the accumulation to FILE after the last sample")
    ap.add_argument("--resume", default="", metavar="FILE", help="continue the accumulation of FILE; --spp is the total")
    ap.add_argument("--aperture", type=float, default=0.0, metavar="R", help="thin-lens aperture radius in world units (0 = pinhole); with --resume, repeat the lens options of the run that wrote the checkpoint")
    focus = ap.add_mutually_exclusive_group()
    focus.add_argument("--focus", type=float, default=None, metavar="D", help="view-space depth of the plane in focus")
    focus.add_argument("--focus-pixel", default=None, metavar="X,Y", help="focus on what this image position sees (default: the image centre)")
    ap.add_argument("--blades", type=int, default=0, metavar="N", help="0 = circular aperture, 3..16 = polygon")
    ap.add_argument("--blade-rotation", type=float, default=0.0, metavar="DEG")
    ap.add_argument("--bake", type=int, nargs=2, default=None, metavar=("W", "H"), help="render into a W x H UV atlas instead of through the camera")
    ap.add_argument("--bake-uv", type=int, choices=[0, 1], default=0, help="the UV set that addresses the atlas")
    ap.add_argument("--bake-instance", type=int, default=-1, metavar="N", help="bake one row of the instance table (default: every instance with the UV set)")
    ap.add_argument("--surface-offset", type=float, default=None, metavar="D", help="the rays start D world units above the surface (default: 1e-4 of the scene's bounding diagonal)")
    ap.add_argument("--dilate", type=int, default=0, metavar="N", help="with --bake: fill N texels (1..64) beyond the charts' borders")
    ap.add_argument("--probes", default=None, metavar="X,Y,Z;...", help="render an atlas of octahedral light probes at these world-space positions instead of through the camera")
    ap.add_argument("--probe-res", type=int, default=32, metavar="N", help="each probe is an N x N map (a multiple of 16 in 16..1024)")
    ap.add_argument("--probe-sh", default="", metavar="OUT.npy", help="with --probes: write the probes' spherical-harmonic coefficients [probes, 9, 3]")
    ap.add_argument("--irradiance", action="store_true", help="with --probe-sh: irradiance coefficients (bands scaled by pi, 2 pi / 3, pi / 4) instead of radiance")
    ap.add_argument("--matte", default=None, choices=["instance", "material"], help="accumulate ID mattes of the instances or of the materials")
    ap.add_argument("--matte-ranks", type=int, default=6, choices=[2, 4, 6, 8], metavar="K", help="(id, coverage) pairs per pixel: 2, 4, 6 or 8")
    ap.add_argument("--matte-out", default="", metavar="PREFIX", help="with --matte: PREFIX_00.exr ... (one per layer) and the manifest PREFIX.json")
    ap.add_argument("--motion-out", default="", metavar="FILE", help="write the motion-vector pass (.exr: 32-bit float RGBA; .npy); needs --prev-time")
    ap.add_argument("--prev-time", type=float, default=None, metavar="T", help="with --motion-out or --motion-blur: the animation time of the previous frame")
    ap.add_argument("--variance-out", default="", metavar="PREFIX", help="write PREFIX.exr (32-bit float RGBA; PREFIX.npy if it ends in .npy): the variance of each pixel's mean")
    ap.add_argument("--noise-target", type=float, default=None, metavar="X", help="stop tracing once no tile's relative standard error exceeds X (or at --spp)")
    ap.add_argument("--sequence", default=None, metavar="T0:T1:FPS", help="render numbered frames of --animation from T0 to T1")
    ap.add_argument("--temporal", action="store_true", help="with --sequence: pt_denoise, then pt_reproject onto the previous frame")
    ap.add_argument("--motion-blur", type=float, default=None, metavar="SHUTTER", help="blur the finished frame along its motion vectors; SHUTTER in (0, 2]; needs --sequence or --prev-time")
    ap.add_argument("--blur-radius", type=float, default=None, metavar="R", help="with --motion-blur: cap of the half streak in pixels (1..64, default 32)")
    ap.add_argument("--blur-taps", type=int, default=None, metavar="N", help="with --motion-blur: taps along the streak (2..64, default 16)")
    ap.add_argument("--bloom", type=float, nargs="?", const=0.01, default=None, metavar="STRENGTH", help="add the reference's bloom to the finished frame; STRENGTH >= 0 (0.01 unless given)")
    ap.add_argument("--bloom-radius", type=int, default=None, metavar="N", help="with --bloom: pyramid levels (0..8, default 4)")
    ap.add_argument("--bloom-threshold", type=float, default=None, metavar="T", help="with --bloom: only what is brighter than T glows (default 0 = everything, as upstream)")
    ap.add_argument("--env-cubes", default="", metavar="PREFIX", help="with --env: write the environment's GGX chain and diffuse cube (pt_env_filter) as PREFIX_ggx_<level>.npy and PREFIX_diffuse.npy")
    a = ap.parse_args()
    if a.env_cubes and not a.env:
        ap.error("--env-cubes needs --env FILE")
    if a.bloom is None and (a.bloom_radius is not None or a.bloom_threshold is not None):
        ap.error("--bloom-radius and --bloom-threshold need --bloom [STRENGTH]")
    if a.bloom is not None:
        if not (math.isfinite(a.bloom) and a.bloom >= 0.0):
            ap.error("--bloom takes a finite strength >= 0")
        if a.bloom_radius is not None and not (0 <= a.bloom_radius <= 8):
            ap.error("--bloom-radius takes 0..8 levels")
        if a.bloom_threshold is not None and not (math.isfinite(a.bloom_threshold) and a.bloom_threshold >= 0.0):
            ap.error("--bloom-threshold takes a finite T >= 0")
        if a.bake is not None or a.probes is not None:
            ap.error("--bloom goes with neither --bake nor --probes: an atlas is not a picture")
    if a.motion_out and a.prev_time is None:
        ap.error("--motion-out FILE needs --prev-time T")
    if a.prev_time is not None and not (a.motion_out or a.motion_blur is not None):
        ap.error("--prev-time T goes with --motion-out FILE or --motion-blur SHUTTER")
    if a.noise_target is not None and not (math.isfinite(a.noise_target) and a.noise_target >= 0.0):
        ap.error("--noise-target takes a finite X >= 0")
    if (a.variance_out or a.noise_target is not None) and (a.checkpoint or a.resume or a.sequence is not None):
        ap.error("--variance-out and --noise-target go with none of --checkpoint, --resume, --sequence: the variance is not part of a checkpoint")
    if a.denoise_variance is not None and (a.denoise is not None or a.sequence is not None or a.checkpoint or a.resume):
        ap.error("--denoise-variance goes with none of --denoise, --sequence, --checkpoint, --resume: one filter a frame, and the variance is not part of a checkpoint")
    if a.denoise_variance is not None and not (0 <= a.denoise_variance <= 6):
        ap.error("--denoise-variance takes 0..6 passes")
    if a.motion_blur is None and (a.blur_radius is not None or a.blur_taps is not None):
        ap.error("--blur-radius and --blur-taps need --motion-blur SHUTTER")
    if a.motion_blur is not None:
        if a.sequence is None and a.prev_time is None:
            ap.error("--motion-blur needs motion vectors: give --sequence T0:T1:FPS, or --prev-time T for a single frame")
        if not (0.0 < a.motion_blur <= 2.0):
            ap.error("--motion-blur takes a shutter in (0, 2]")
        if a.blur_radius is not None and not (1.0 <= a.blur_radius <= 64.0):
            ap.error("--blur-radius takes 1..64 pixels")
        if a.blur_taps is not None and not (2 <= a.blur_taps <= 64):
            ap.error("--blur-taps takes 2..64")
    if a.temporal and a.sequence is None:
        ap.error("--temporal needs --sequence T0:T1:FPS")
    sequence_times = None
    if a.sequence is not None:
        try:
            sequence_times = sequence_frames(a.sequence)
        except ValueError:
            ap.error("--sequence takes T0:T1:FPS with T1 >= T0 and FPS > 0")
    if (a.prev_time is not None or sequence_times is not None) and (a.bake is not None or a.probes is not None):
        ap.error("motion vectors describe camera rays: --motion-out, --motion-blur and --sequence go with neither --bake nor --probes")
    if sequence_times is not None and (a.adaptive is not None or a.matte is not None or a.checkpoint or a.resume or a.motion_out):
        ap.error("--sequence goes with none of --adaptive, --matte, --checkpoint, --resume, --motion-out")
    if a.prev_time is not None and (a.checkpoint or a.resume):
        ap.error("--motion-out and --motion-blur go with neither --checkpoint nor --resume: the pass is not part of a checkpoint")
    if a.matte is None and (a.matte_out or a.matte_ranks != 6):
        ap.error("--matte-ranks and --matte-out need --matte instance|material")
    if a.matte is not None and not a.matte_out:
        ap.error("--matte needs --matte-out PREFIX")
    if a.matte is not None and (a.checkpoint or a.resume):
        ap.error("--matte goes with neither --checkpoint nor --resume: the layers are not part of a checkpoint")
    if a.bake is None and (a.dilate or a.surface_offset is not None or a.bake_instance != -1 or a.bake_uv != 0):
        ap.error("--bake-uv, --bake-instance, --surface-offset and --dilate need --bake W H")
    if a.bake is not None and a.aperture > 0:
        ap.error("--aperture does not apply to --bake: a bake has no lens")

    probe_positions = None
    if a.probes is not None:
        if a.bake is not None or a.aperture > 0:
            ap.error("--probes goes with neither --bake nor --aperture")
        try:
            probe_positions = np.array([[float(v) for v in item.split(",")] for item in a.probes.split(";") if item.strip()], np.float32)
            assert probe_positions.ndim == 2 and probe_positions.shape[1] == 3 and len(probe_positions) >= 1
        except (ValueError, AssertionError):
            ap.error("--probes takes positions as \"x,y,z;x,y,z;...\"")
    elif a.probe_sh or a.irradiance or a.probe_res != 32:
        ap.error("--probe-res, --probe-sh and --irradiance need --probes")
    if a.irradiance and not a.probe_sh:
        ap.error("--irradiance needs --probe-sh OUT.npy")

    import torch
    from gltf_renderer_amd import abi, camera, gltf
    from gltf_renderer_amd.renderer import Renderer

    r = Renderer(0)
    sc = gltf.GltfScene(a.path)
    sc.upload(r)

    def pose(t):
        """The scene at animation time t in the context: node transforms, skinning, the instance table.  Returns the light count."""
        if a.animation >= 0:
            sc.animate(a.animation, t)
        sc.calculate_global_transforms(0)
        return sc.frame(r, 0)

    if a.prev_time is not None:                                          # the previous frame's pose first: its triangles are the snapshot
        pose(a.prev_time)
        r.motion_snapshot()
    lights = pose(sequence_times[0] if sequence_times is not None else a.time)
    # bounds from the loaded streams and node transforms
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    c = sc.counts()
    first_flat, f = {}, 0
    for m in range(c.meshes):
        first_flat[m] = f
        while f < c.primitives and sc.primitive(f)["mesh"] == m:
            f += 1
    for n in range(c.nodes):
        ni = sc.node(n)
        if ni.mesh < 0:
            continue
        g = np.array(ni.global_transform[:], np.float64).reshape(4, 4).T
        k = first_flat[ni.mesh]
        while k < c.primitives and sc.primitive(k)["mesh"] == ni.mesh:
            p = sc.primitive(k)["position"]
            if p is not None and len(p):
                w = p.astype(np.float64) @ g[:3, :3].T + g[:3, 3]
                lo, hi = np.minimum(lo, w.min(0)), np.maximum(hi, w.max(0))
            k += 1
    centre, radius = (lo + hi) / 2, float(np.linalg.norm(hi - lo)) / 2
    env = None
    if a.env:
        img, _ = gltf.load_rgb32f(a.env)
        env = r.env_create(np.ascontiguousarray(img))
        if a.env_cubes:
            r.env_filter(env)                                            # the reference's sample counts, biases and sizes
            info = r.env_filter_info(env)
            for mip in range(info.ggx_mips):
                np.save("%s_ggx_%d.npy" % (a.env_cubes, mip), r.env_filter_read(env, abi.ENV_FILTER_GGX, mip)[0].view(np.float16))
            np.save(a.env_cubes + "_diffuse.npy", r.env_filter_read(env, abi.ENV_FILTER_DIFFUSE)[0].view(np.float16))
            print("environment cubes: GGX %d^2, %d levels, roughness %s; diffuse %d^2 -> %s_ggx_<level>.npy, %s_diffuse.npy" % (
                info.ggx_resolution, info.ggx_mips, ", ".join("%.4g" % v for v in list(info.ggx_roughness)[:info.ggx_mips]),
                info.diffuse_resolution, a.env_cubes, a.env_cubes))
    st = abi.PtSettings.app_defaults()
    st.max_bounces = a.bounces
    if env is None:
        st.flags &= ~(abi.FLAG_ENVIRONMENT_MAP | abi.FLAG_ENVIRONMENT_MIS)
        st.environment_color[:] = (0.6, 0.7, 0.9)
    r.set_bounce_limit(max(a.bounces, abi.REFERENCE_MAX_BOUNCES))
    w, h = a.bake if a.bake is not None else a.size
    if probe_positions is not None:
        w, h = r.set_probes(probe_positions, a.probe_res, max_distance=max(1000.0, 4.0 * radius))
        print("probes: %d of %d x %d texels, atlas %d x %d" % (len(probe_positions), a.probe_res, a.probe_res, w, h))
    p = abi.PtExecuteParams()
    p.world_to_view[:] = camera.cm(camera.orbit_world_to_view(tuple(centre), 2.2 * radius, a.azimuth, a.inclination))
    p.view_to_clip[:] = camera.cm(camera.view_to_clip(w / h, math.radians(60), 0.01 * radius, 100.0 * radius))
    p.width, p.height, p.light_count = w, h, lights
    p.environment_map = -1 if env is None else env
    p.tile_rank, p.tile_rank_count = 0, 1
    if a.aperture > 0:
        if a.focus is not None:
            focus_distance = a.focus
        else:
            fx, fy = (float(v) for v in a.focus_pixel.split(",")) if a.focus_pixel else (w / 2, h / 2)
            focus_distance = r.focus_at(st, p, fx, fy)
            if focus_distance is None:
                sys.exit("--focus-pixel %g,%g: nothing to focus on there, give another position or --focus D" % (fx, fy))
            print("focus at pixel %g,%g: depth %.6g" % (fx, fy, focus_distance))
        r.set_lens(a.aperture, focus_distance, a.blades, math.radians(a.blade_rotation))
    if a.bake is not None:
        offset = a.surface_offset if a.surface_offset is not None else 1e-4 * 2.0 * radius
        r.set_bake(offset, a.bake_uv, a.bake_instance)
        print("bake %d x %d: UV set %d, %s, surface offset %.6g" % (w, h, a.bake_uv, "every instance" if a.bake_instance < 0 else "instance %d" % a.bake_instance, offset))
    out = r.create_output(w, h)
    aov_albedo = aov_nd = None
    if a.aov or a.denoise is not None or a.denoise_variance is not None or a.temporal:
        aov_albedo, aov_nd = r.create_output(w, h), r.create_output(w, h)
        r.set_aov(aov_albedo, aov_nd)
    matte_layers = None
    if a.matte is not None:
        matte_layers = [r.create_output(w, h) for _ in range(a.matte_ranks // 2)]
        r.set_matte(abi.MATTE_MATERIAL if a.matte == "material" else abi.MATTE_INSTANCE, matte_layers)
    motion = None
    if a.prev_time is not None or sequence_times is not None:            # the camera stands still: the previous matrices are this frame's
        motion = r.create_output(w, h)
        r.set_motion(motion, p.world_to_view[:], p.view_to_clip[:])
    variance = None
    if a.variance_out or a.noise_target is not None or a.denoise_variance is not None:
        variance = r.create_output(w, h)
        r.set_variance(variance)
    blur = None
    if a.motion_blur is not None:
        blur = abi.PtMotionBlurConfig.defaults()
        blur.shutter = a.motion_blur
        if a.blur_radius is not None:
            blur.max_radius = a.blur_radius
        if a.blur_taps is not None:
            blur.taps = a.blur_taps
    bloom = None
    if a.bloom is not None:
        bloom = abi.PtBloomConfig.defaults()
        bloom.strength = a.bloom
        if a.bloom_radius is not None:
            bloom.iterations = a.bloom_radius
        if a.bloom_threshold is not None:
            bloom.threshold = a.bloom_threshold

    def write_frame(path, image):
        if path.lower().endswith(".exr"):
            gltf.write_exr(path, r.readback(image)[..., :3], half=True)  # linear radiance
        elif path.lower().endswith(".pfm"):
            gltf.write_pfm(path, r.readback(image)[..., :3])
        else:
            gltf.write_png(path, r.tonemap(image, want_rgba8=True)[1], 3)   # tone-mapped (AgX + sRGB), ToneMapper.ps.hlsl

    if sequence_times is not None:
        # per frame: snapshot of the pose just rendered, the next pose, --spp samples of a new accumulation with the motion pass beside it,
        # then (--temporal) pt_denoise and pt_reproject onto the previous filtered frame
        prev_color = prev_motion = prev_length = None
        dn = abi.PtDenoiseConfig.default()
        if a.denoise is not None:
            dn.iterations = a.denoise
        for i, t in enumerate(sequence_times):
            if i > 0:
                r.motion_snapshot()
                p.light_count = pose(t)
            st.reset = 1
            for k in range(a.spp):
                p.frame = i * a.spp + k
                r.trace(st, p, out)
                st.reset = 0
            shown = out
            if a.temporal:
                shown = r.denoise(out, aov_albedo, aov_nd, config=dn)
                if prev_color is not None:
                    shown, prev_length = r.reproject(shown, motion, prev_color, prev_motion, prev_length)
                prev_color, prev_motion = shown, motion.clone()
            elif a.denoise is not None:
                shown = r.denoise(out, aov_albedo, aov_nd, config=dn)
            if blur is not None:                                         # after the filters; the history above stays unblurred
                shown = r.motion_blur(shown, motion, config=blur)
            if bloom is not None:                                        # last before tone mapping; into a new image: `shown` may be the history
                shown = r.bloom(shown, config=bloom)
            write_frame(numbered_path(a.out, i), shown)
        torch.cuda.synchronize()
        s = r.stats()
        print("%s: %d frames %s .. %s, t = %.4g .. %.4g, %d spp each%s, last trace %.2f ms" % (a.path, len(sequence_times), numbered_path(a.out, 0),
              numbered_path(a.out, len(sequence_times) - 1), sequence_times[0], sequence_times[-1], a.spp, (", denoised and reprojected" if a.temporal else "") + (", motion blur at shutter %g" % a.motion_blur if blur is not None else "") + (", bloom at strength %g" % a.bloom if bloom is not None else ""), s.trace_ms))
        return
    adaptive_cfg = None if a.adaptive is None else (min(a.min_spp, a.spp), a.spp, a.adaptive)
    if adaptive_cfg is not None:
        r.set_samples_per_trace(min(a.batch, 64))
        r.set_adaptive(*adaptive_cfg)
    first = 0
    if a.resume:
        # options first, as for a fresh run; then the state.  A file that does not fit is refused before anything is loaded.
        blob = open(a.resume, "rb").read()
        try:
            info = Renderer.accum_inspect(blob)
        except Exception:
            sys.exit("--resume %s: not a valid accumulation checkpoint" % a.resume)
        why = resume_mismatch(info, (w, h), aov_albedo is not None, adaptive_cfg, (abi.ACCUM_ALBEDO, abi.ACCUM_NORMAL_DEPTH, abi.ACCUM_ADAPTIVE))
        if why:
            sys.exit("--resume %s: %s" % (a.resume, why))
        if info.accumulated_frames > a.spp:
            sys.exit("--resume %s: it already holds %d samples, --spp (the total) is %d" % (a.resume, info.accumulated_frames, a.spp))
        r.accum_load(blob, out, aov_albedo, aov_nd)
        first = int(info.next_frame)
        print("resumed %s: %d samples, continuing with frame %d" % (a.resume, info.accumulated_frames, first))
    noise = None                                                         # (tile_mean, tile_max, summary) of the last pt_noise_estimate
    if a.adaptive is None and a.noise_target is not None:
        # trace batches until no tile's error exceeds the target or the pixels hold --spp samples
        traced, batch = 0, max(1, min(a.batch, 64))
        while traced < a.spp:
            r.set_samples_per_trace(min(batch, a.spp - traced))
            p.frame = traced
            r.trace(st, p, out)
            traced += min(batch, a.spp - traced)
            if traced >= 2:
                noise = r.noise_estimate(out, variance, samples=traced, threshold=a.noise_target)
                if noise[2].max <= a.noise_target:
                    break
        uniform_samples = next_frame = traced
    elif a.adaptive is None:
        done = info.accumulated_frames if a.resume else 0
        for frame in range(first, first + a.spp - done):
            p.frame = frame
            r.trace(st, p, out)
        next_frame = first + a.spp - done
        uniform_samples = a.spp
    else:
        # trace batches until no tile is active or every tile holds --spp samples
        frame, active = first, (r.adaptive_read(w, h)[0] if a.resume else 1)
        done = info.accumulated_frames if a.resume else 0
        while active and frame - first < a.spp - done:
            p.frame = frame
            r.trace(st, p, out)
            frame += min(a.batch, 64)
            active = r.adaptive_read(w, h)[0]
            if a.noise_target is not None:
                noise = r.noise_estimate(out, variance, tile_samples=r.adaptive_read(w, h)[1], threshold=a.noise_target)
                if noise[2].tiles_estimated and noise[2].max <= a.noise_target:
                    break
        next_frame = frame
        _, samples, _, _ = r.adaptive_read(w, h)
        pix = np.zeros((samples.shape[0] * abi.TILE, samples.shape[1] * abi.TILE), np.int64)
        pix[:h, :w] = 1
        pix = pix.reshape(samples.shape[0], abi.TILE, samples.shape[1], abi.TILE).sum(axis=(1, 3))
        used, full = int((samples.astype(np.int64) * pix).sum()), w * h * a.spp
        print("adaptive %.4g: %d of %d tile-samples (%d tiles x %d spp), %d pixel-samples = %.1f %% of uniform; tile counts %d..%d"
              % (a.adaptive, int(samples.sum()), samples.size * a.spp, samples.size, a.spp, used, 100.0 * used / full, samples.min(), samples.max()))
        if a.sample_map:
            grey = np.repeat(np.repeat((255.0 * samples / a.spp).astype(np.uint8), abi.TILE, 0), abi.TILE, 1)[:h, :w]
            gltf.write_png(a.sample_map, np.dstack([grey, grey, grey, np.full_like(grey, 255)]), 3)
    torch.cuda.synchronize()
    if variance is not None:
        # the counts the target stands for: the tiles' own under adaptive sampling, else the samples traced
        counts = r.adaptive_read(w, h)[1] if a.adaptive is not None else np.full(((h + abi.TILE - 1) // abi.TILE, (w + abi.TILE - 1) // abi.TILE), uniform_samples, np.uint32)
        if counts.max() >= 2:
            tile_mean, tile_max, ns = r.noise_estimate(out, variance, tile_samples=counts, threshold=a.noise_target or 0.0)
            print("noise: relative standard error mean %.4g, max %.4g over %d of %d tiles%s; samples %d..%d" % (ns.mean, ns.max, ns.tiles_estimated, ns.tiles,
                  ("; %d tiles above the target %.4g" % (ns.tiles_above, a.noise_target)) if a.noise_target is not None else "", counts.min(), counts.max()))
        else:
            print("noise: a single sample has no variance")
        if a.variance_out:
            per_pixel = np.repeat(np.repeat(counts, abi.TILE, 0), abi.TILE, 1)[:h, :w].astype(np.float32)
            with np.errstate(all="ignore"):
                of_mean = np.where(per_pixel[..., None] >= 2, r.readback(variance) / (per_pixel[..., None] - 1.0), 0.0).astype(np.float32)
            path = a.variance_out if a.variance_out.lower().endswith((".npy", ".exr")) else a.variance_out + ".exr"
            if path.lower().endswith(".npy"):
                np.save(path, of_mean)
            else:
                write_exr_rgba32f(path, of_mean)
            print("variance of the mean (rgb per channel, a of the channel sum): %s" % path)
    if a.checkpoint:                                                     # before the denoiser: the state is the noisy accumulation
        blob = r.accum_save(w, h, out, aov_albedo, aov_nd, next_frame=next_frame)
        with open(a.checkpoint, "wb") as f:
            f.write(blob)
        print("checkpoint %s: %d bytes, %d samples, next frame %d" % (a.checkpoint, len(blob), Renderer.accum_inspect(blob).accumulated_frames, next_frame))
    if a.denoise is not None:
        _, noisy8 = r.tonemap(out, want_rgba8=True)
        gltf.write_png(noisy_path(a.out), noisy8, 3)
        cfg = abi.PtDenoiseConfig.default()
        cfg.iterations = a.denoise
        r.denoise(out, aov_albedo, aov_nd, out=out, config=cfg)          # in place: the AOVs are only read
    if a.denoise_variance is not None:                                   # where --denoise runs; `counts` is what the noise report above used
        _, noisy8 = r.tonemap(out, want_rgba8=True)
        gltf.write_png(noisy_path(a.out), noisy8, 3)
        cfg = abi.PtDenoiseVarianceConfig.default()
        cfg.iterations = a.denoise_variance
        if counts.max() >= 2:
            r.denoise_variance(out, aov_albedo, aov_nd, variance, tile_samples=counts, out=out, config=cfg)      # in place: the rest is only read
        else:
            print("--denoise-variance: a single sample has no variance, the frame stays as it is")
    if a.bake is not None:
        cover = r.bake_coverage(w, h)[0] >= 0
        print("bake: %d of %d texels covered (%.1f %%)" % (int(cover.sum()), w * h, 100.0 * cover.mean()))
        if a.dilate:
            r.bake_dilate(out, a.dilate)
    if blur is not None:                                                 # after the denoiser, before tone mapping
        out = r.motion_blur(out, motion, config=blur)
        print("motion blur (t = %.4g -> %.4g): shutter %g, half streak <= %g px, %d taps" % (a.prev_time, a.time, blur.shutter, blur.max_radius, blur.taps))
    if bloom is not None:                                                # last before tone mapping
        out = r.bloom(out, out=out, config=bloom)                        # in place: the last step reads the pyramid and its own pixel
        print("bloom: strength %g, %d levels, threshold %g" % (bloom.strength, bloom.iterations, bloom.threshold))
    if a.probe_sh:
        np.save(a.probe_sh, r.probe_project(out, abi.PROBE_SH_IRRADIANCE if a.irradiance else abi.PROBE_SH_RADIANCE))
        print("probe SH (%s): %s" % ("irradiance" if a.irradiance else "radiance", a.probe_sh))
    _, rgba8 = r.tonemap(out, want_rgba8=True)
    if a.out.lower().endswith(".exr"):
        gltf.write_exr(a.out, r.readback(out)[..., :3], half=True)       # linear radiance
    elif a.out.lower().endswith(".pfm"):
        gltf.write_pfm(a.out, r.readback(out)[..., :3])
    else:
        gltf.write_png(a.out, rgba8, 3)                                  # tone-mapped (AgX + sRGB), ToneMapper.ps.hlsl
    if a.motion_out:
        mv = r.readback(motion)
        if a.motion_out.lower().endswith(".npy"):
            np.save(a.motion_out, mv)
        else:
            write_exr_rgba32f(a.motion_out, mv)
        moving = mv[..., 3] > 0
        print("motion (t = %.4g -> %.4g): %s, %d of %d pixels covered, largest vector %.2f px" % (a.prev_time, a.time, a.motion_out, int(moving.sum()), w * h,
              float(np.hypot(mv[..., 0], mv[..., 1])[moving].max()) if moving.any() else 0.0))
    if matte_layers is not None:
        seen = set()
        for j, layer in enumerate(matte_layers):
            img = r.readback(layer)
            write_exr_rgba32f("%s_%02d.exr" % (a.matte_out, j), img)
            seen |= set(np.unique(img.view(np.uint32)[..., 0::2]).tolist()) - {0}
        # the default names of the table's rows, up to the last row a pixel shows (the scene header carries no names)
        manifest, rows = {}, 0
        while seen and rows < (1 << 20):
            name = "%s_%d" % (a.matte, rows)
            manifest[name] = "%08x" % Renderer.matte_id(name)
            seen.discard(int(manifest[name], 16))
            rows += 1
        with open(a.matte_out + ".json", "w") as f:
            json.dump(manifest, f, indent=1)
        print("matte (%s, %d ranks): %s_00.exr .. %s_%02d.exr, manifest %s.json (%d names)" % (a.matte, a.matte_ranks, a.matte_out, a.matte_out, len(matte_layers) - 1, a.matte_out, rows))
    if a.aov:
        opaque = np.full((h, w, 1), 255, np.uint8)
        alb8, nrm8, depth = aov_images(r.readback(aov_albedo), r.readback(aov_nd))
        gltf.write_png(a.aov + "_albedo.png", np.dstack([alb8, opaque]), 3)
        gltf.write_png(a.aov + "_normal.png", np.dstack([nrm8, opaque]), 3)
        np.save(a.aov + "_depth.npy", depth)
    s = r.stats()
    print("%s: %d triangles, %d lights, %d spp, %.2f ms/frame, %.0f Mrays/s -> %s" % (a.path, s.bvh_triangles, lights, a.spp, s.trace_ms, s.rays / max(s.trace_ms, 1e-9) / 1e3 / max(a.spp, 1) * 1.0, a.out))


if __name__ == "__main__":
    main()
