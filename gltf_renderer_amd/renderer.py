"""ctypes binding of libmipt.so (include/mipt.h).  No CPU fallback: if the HIP library is missing or
its symbols do not match the header, importing the Renderer fails loudly.

PyTorch is used only as plumbing: the caller-owned output image is a CUDA(HIP) tensor and the
library enqueues on torch's current stream, so torch.distributed (RCCL) can reduce the image.
"""
import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmipt.so")

EXPORTS = list(abi.PROTOTYPES)      # every symbol include/mipt.h declares
MiptError = abi.MiptError


_LIB = None


def load_library():
    global _LIB
    if _LIB is not None:
        return _LIB
    # MIPT_LIBRARY: a tuning build of the same library (tools/build_variant.sh) for A/B runs; never another implementation
    lib_path = os.environ.get("MIPT_LIBRARY") or LIB_PATH
    if not os.path.exists(lib_path):
        raise MiptError("libmipt.so not found at %s: build it with `make -C gltf_renderer_amd/csrc` "
                        "(or __graft_entry__.build()); there is no CPU fallback" % lib_path)
    # One HIP runtime per process: PyTorch ships its own libamdhip64, and whichever copy is mapped first serves both.  Import
    # torch BEFORE libmipt.so so that it is torch's copy (loading /opt/rocm's first makes later device queries fail).
    import torch  # noqa: F401
    L = C.CDLL(lib_path)
    abi.bind(L, abi.PROTOTYPES, "include/mipt.h")
    if L.pt_abi_version() != 2:
        raise MiptError("libmipt.so ABI version mismatch")
    _LIB = L
    return L


def sheen_lut():
    return np.fromfile(os.path.join(_HERE, "data", "sheen_e_16x16.f32"), dtype=np.float32)


def _p(a):
    """A numpy array's host pointer; None for None."""
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _dp(t):
    """A tensor's device pointer; None for None."""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _ref(struct):
    """byref of a config structure; None (= the library's defaults) for None."""
    return C.byref(struct) if struct is not None else None


def _tiles(h, w):
    return (h + abi.TILE - 1) // abi.TILE, (w + abi.TILE - 1) // abi.TILE


def _tile_samples(tile_samples, h, w):
    """The per-tile sample counts of an (h, w) image as a contiguous uint32 array, one per tile; None for None."""
    if tile_samples is None:
        return None
    ts = np.ascontiguousarray(tile_samples, np.uint32)
    ty, tx = _tiles(h, w)
    assert ts.size == ty * tx
    return ts


class Renderer:
    """Host mirror of the reference's hot-path objects behind one context:
    Pathtracer::{Init, PathtraceScene, Shutdown} (Source/Pathtracer.h:104-106),
    GpuSkin::{Create, Run} (Source/GpuSkin.h:17-19), EnvironmentMap::CreateEnvironmentMap."""

    def __init__(self, device=0, stream=None):
        import torch
        if not torch.cuda.is_available():
            raise MiptError("no HIP device visible: the path tracer runs on MI355X only (no CPU fallback)")
        self.torch = torch
        self.L = load_library()
        self.device = device
        torch.cuda.set_device(device)
        self.stream = torch.cuda.current_stream(device).cuda_stream if stream is None else stream
        lut = sheen_lut()
        h = C.c_void_p()
        rc = self.L.pt_create(device, C.c_void_p(self.stream), _p(lut), C.byref(h))
        if rc != 0:
            raise MiptError("pt_create failed: %d" % rc)
        self.h = h

    # ---- the contract of every image argument, said once
    def _image(self, x, like=None, optional=False):
        """x is a float32 CUDA contiguous (H, W, 4) tensor -- of like's shape, if one is given; None passes if optional.  Returns x."""
        if x is None and optional:
            return x
        assert x.is_cuda and x.is_contiguous() and x.dtype == self.torch.float32 and x.dim() == 3 and x.shape[2] == 4
        assert like is None or x.shape == like.shape
        return x

    def _plane(self, x, h, w, optional=False):
        """x is a float32 CUDA contiguous (h, w) tensor; None passes if optional.  Returns x."""
        assert (x is None and optional) or (x.is_cuda and x.is_contiguous() and x.dtype == self.torch.float32 and tuple(x.shape) == (h, w))
        return x

    def _check(self, rc):
        if rc != 0:
            raise MiptError("%d: %s" % (rc, self.L.pt_last_error(self.h).decode()))

    def close(self):
        if getattr(self, "h", None):
            self.L.pt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- resources
    def buffer_create(self, data, fmt, nbytes=None):
        out = C.c_int()
        if data is None:
            self._check(self.L.pt_buffer_create(self.h, None, nbytes, fmt, C.byref(out)))
        else:
            a = np.ascontiguousarray(data)
            self._check(self.L.pt_buffer_create(self.h, _p(a), a.nbytes, fmt, C.byref(out)))
        return out.value

    def buffer_update(self, handle, data):
        a = np.ascontiguousarray(data)
        self._check(self.L.pt_buffer_update(self.h, handle, _p(a), a.nbytes))

    def buffer_read(self, handle, dtype, count):
        out = np.zeros(count, dtype)
        self._check(self.L.pt_buffer_read(self.h, handle, _p(out), out.nbytes))
        return out

    def buffer_destroy(self, handle):
        self._check(self.L.pt_buffer_destroy(self.h, handle))

    def texture_destroy(self, handle):
        self._check(self.L.pt_texture_destroy(self.h, handle))

    def env_destroy(self, env):
        self._check(self.L.pt_env_destroy(self.h, env))

    def texture_create(self, rgba8, srgb):
        a = np.ascontiguousarray(rgba8, dtype=np.uint8)
        h, w = a.shape[:2]
        out = C.c_int()
        self._check(self.L.pt_texture_create(self.h, _p(a), w, h, int(bool(srgb)), C.byref(out)))
        return out.value

    def sampler_create(self, address_u, address_v, min_filter, mag_filter):
        d = abi.PtSamplerDesc(address_u, address_v, min_filter, mag_filter)
        out = C.c_int()
        self._check(self.L.pt_sampler_create(self.h, C.byref(d), C.byref(out)))
        return out.value

    def set_materials(self, materials):
        arr = (abi.PtMaterial * len(materials))(*materials)
        self._check(self.L.pt_scene_set_materials(self.h, C.byref(arr), len(materials)))

    def set_lights(self, lights):
        if len(lights) == 0:
            self._check(self.L.pt_scene_set_lights(self.h, None, 0))
            return
        arr = (abi.PtLight * len(lights))(*lights)
        self._check(self.L.pt_scene_set_lights(self.h, C.byref(arr), len(lights)))

    def set_instances(self, instances):
        arr = (abi.PtInstanceDesc * len(instances))(*instances)
        self._check(self.L.pt_scene_set_instances(self.h, C.byref(arr), len(instances)))

    def env_create(self, equirect_rgb32f):
        a = np.ascontiguousarray(equirect_rgb32f, dtype=np.float32)
        h, w = a.shape[:2]
        out = C.c_int()
        self._check(self.L.pt_env_create(self.h, _p(a), w, h, C.byref(out)))
        return out.value

    def env_read(self, env):
        n = C.c_int()
        self._check(self.L.pt_env_read(self.h, env, C.byref(n), None, None))
        cube = np.zeros((6, n.value, n.value, 4), np.uint16)
        pyr = np.zeros(sum((1024 >> i) ** 2 for i in range(11)), np.float32)
        self._check(self.L.pt_env_read(self.h, env, C.byref(n), _p(cube), _p(pyr)))
        return n.value, cube, pyr

    def env_filter(self, env, config=None):
        """The environment's GGX chain and diffuse cube (include/mipt.h pt_env_filter); config: abi.PtEnvFilterConfig, None = the reference's
        values.  Asynchronous."""
        self._check(self.L.pt_env_filter(self.h, env, _ref(config)))

    def env_filter_info(self, env):
        info = abi.PtEnvFilterInfo()
        self._check(self.L.pt_env_filter_info_get(self.h, env, C.byref(info)))
        return info

    def env_filter_read(self, env, which, mip=0, host=True):
        """One level of the GGX chain (which = abi.ENV_FILTER_GGX) or the diffuse cube (abi.ENV_FILTER_DIFFUSE): (the (6, n, n, 4) uint16
        RGBA16F texels, or None with host=False; the context-owned device pointer to them as an int)."""
        n, dev = C.c_int(), C.c_void_p()
        self._check(self.L.pt_env_filter_read(self.h, env, which, mip, C.byref(n), None, None))
        texels = np.zeros((6, n.value, n.value, 4), np.uint16) if host else None
        self._check(self.L.pt_env_filter_read(self.h, env, which, mip, C.byref(n), _p(texels), C.byref(dev)))
        return texels, dev.value

    def set_bounce_limit(self, limit):
        self._check(self.L.pt_set_bounce_limit(self.h, limit))

    def set_samples_per_trace(self, samples):
        """Sample batch: one trace() then stands for `samples` consecutive frames (bit-identical to issuing them one by one)."""
        self._check(self.L.pt_set_samples_per_trace(self.h, int(samples)))

    def set_adaptive(self, min_samples, max_samples, threshold, enable=True):
        """Tile-level adaptive sampling (include/mipt.h pt_set_adaptive): on accumulating calls, a 16x16 tile stops getting samples
        once it holds max_samples (or settings.max_accumulated_frames), or at least min_samples with its error <= threshold.
        The next trace() starts a new accumulation."""
        cfg = abi.PtAdaptiveConfig(int(bool(enable)), int(min_samples), int(max_samples), float(threshold))
        self._check(self.L.pt_set_adaptive(self.h, C.byref(cfg)))

    def adaptive_read(self, width, height):
        """State after the last adaptive trace: (active tile count, samples (tiles_y, tiles_x) uint32, error (tiles_y, tiles_x)
        float32, half image (height, width, 4) float32).  Tiles another rank renders read 0."""
        ty, tx = _tiles(height, width)
        active = C.c_int32()
        samples = np.zeros((ty, tx), np.uint32)
        error = np.zeros((ty, tx), np.float32)
        half = np.zeros((height, width, 4), np.float32)
        self._check(self.L.pt_adaptive_read(self.h, width, height, C.byref(active), _p(samples), _p(error), _p(half)))
        return active.value, samples, error, half

    def set_aov(self, albedo=None, normal_depth=None):
        """First-hit AOVs (include/mipt.h pt_set_aov): albedo (rgb, coverage) and normal_depth (signed world-space shading normal,
        hit distance) are float32 CUDA tensors (H, W, 4) like the output, caller-owned; either may be None, both None turns AOVs off.
        They accumulate with the output, sample for sample.  The next trace() starts a new accumulation."""
        for t in (albedo, normal_depth):
            self._image(t, optional=True)
        cfg = abi.PtAovConfig(int(albedo is not None or normal_depth is not None), _dp(albedo), _dp(normal_depth))
        self._check(self.L.pt_set_aov(self.h, C.byref(cfg)))
        self._aov = (albedo, normal_depth)           # the library keeps the pointers: keep the tensors alive with the renderer

    def denoise(self, color, albedo, normal_depth, out=None, config=None):
        """The a-trous filter over the first-hit AOVs (include/mipt.h pt_denoise): color, albedo and normal_depth are float32 CUDA tensors
        (H, W, 4) -- the output of trace() and the targets of set_aov(), or any images of that layout.  out: where the result goes (None = a
        new tensor; `color` itself filters in place); config: abi.PtDenoiseConfig (None = the defaults).  Asynchronous on the context's
        stream.  Returns the output tensor."""
        if out is None:
            out = self.torch.empty_like(color)
        for x in (color, albedo, normal_depth, out):
            self._image(x, like=color)
        h, w = color.shape[:2]
        self._check(self.L.pt_denoise(self.h, _ref(config), _dp(color), _dp(albedo), _dp(normal_depth), w, h, _dp(out)))
        return out

    # ---- saving and resuming an accumulation (include/mipt.h pt_accum_save / pt_accum_load / pt_accum_inspect)
    def _accum_images(self, output, albedo, normal_depth):
        return abi.PtAccumImages(*[_dp(self._image(t, optional=True)) for t in (output, albedo, normal_depth)])

    def accum_save(self, width, height, output, albedo=None, normal_depth=None, rank=0, world=1, next_frame=0):
        """The accumulation as one bytes blob: the images given (the output of trace() and, if AOVs are on, the targets of set_aov()), the
        count and camera and, with adaptive sampling, the tile state.  rank / world: the tile shard traced (the blob holds the rank's
        tiles).  next_frame: the frame number to continue with, kept for the caller.  Synchronises the stream."""
        assert output is not None and tuple(output.shape[:2]) == (height, width)
        img = self._accum_images(output, albedo, normal_depth)
        need = C.c_size_t()
        self._check(self.L.pt_accum_save(self.h, C.byref(img), width, height, rank, world, next_frame, None, 0, C.byref(need)))
        blob = bytearray(need.value)
        buf = (C.c_ubyte * need.value).from_buffer(blob)
        self._check(self.L.pt_accum_save(self.h, C.byref(img), width, height, rank, world, next_frame, buf, need.value, C.byref(need)))
        del buf
        return bytes(blob)

    def accum_load(self, blob, output, albedo=None, normal_depth=None):
        """Puts a blob of accum_save() into this renderer and the given tensors (fresh ones, of the blob's size): call it after the scene
        upload and set_adaptive() / set_aov() / set_samples_per_trace() as for a fresh run; trace() with the saved camera and reset = 0
        then continues from the blob's next_frame.  Returns the blob's abi.PtAccumInfo."""
        info = self.accum_inspect(blob)
        for t in (output, albedo, normal_depth):
            assert t is None or tuple(t.shape[:2]) == (info.height, info.width), "target size differs from the blob's"
        img = self._accum_images(output, albedo, normal_depth)
        self._check(self.L.pt_accum_load(self.h, bytes(blob), len(blob), C.byref(img)))
        return info

    @staticmethod
    def accum_inspect(blob):
        """What a blob holds (abi.PtAccumInfo); raises MiptError for one that is malformed.  No GPU call."""
        info = abi.PtAccumInfo()
        rc = load_library().pt_accum_inspect(bytes(blob), len(blob), C.byref(info))
        if rc != 0:
            raise MiptError("%d: not a valid accumulation blob" % rc)
        return info

    def set_lens(self, aperture_radius, focus_distance, blades=0, blade_rotation=0.0, enable=True):
        """Thin-lens depth of field (include/mipt.h pt_set_lens): aperture_radius in world units (0 = the pinhole, bit for bit),
        focus_distance = view-space depth of the plane in focus, blades = 0 for a circular aperture or 3..16 for a polygon whose vertex 0
        sits at blade_rotation radians.  The next trace() starts a new accumulation.  The lens is not part of an accum_save() blob: set the
        same lens before accum_load()."""
        cfg = abi.PtLensConfig(int(bool(enable)), float(aperture_radius), float(focus_distance), int(blades), float(blade_rotation))
        self._check(self.L.pt_set_lens(self.h, C.byref(cfg)))

    def set_bake(self, surface_offset, tex_coord=0, instance=-1, enable=True):
        """Texture-space baking (include/mipt.h pt_set_bake): trace() renders into the width x height atlas addressed by UV set tex_coord
        of every instance that has it (instance = -1) or of one instance-table row; every ray starts surface_offset (world units) above
        its texel's surface point.  The next trace() starts a new accumulation.  Wavefront mode only.  The bake is not part of an
        accum_save() blob: set the same bake before accum_load()."""
        cfg = abi.PtBakeConfig(int(bool(enable)), int(tex_coord), int(instance), float(surface_offset))
        self._check(self.L.pt_set_bake(self.h, C.byref(cfg)))

    def bake_coverage(self, width, height):
        """The coverage map of the last bake trace() (pt_bake_coverage): (instance [H, W] int32, -1 where no triangle covers;
        primitive [H, W] uint32, the triangle within the instance)."""
        inst = np.zeros((height, width), np.int32)
        prim = np.zeros((height, width), np.uint32)
        self._check(self.L.pt_bake_coverage(self.h, width, height, _p(inst), _p(prim)))
        return inst, prim

    def bake_dilate(self, image, passes):
        """pt_bake_dilate: fills the uncovered texels of a device image (create_output) from their covered neighbours, `passes` texels
        deep, in place; for the atlas size of the last bake trace()."""
        self._check(self.L.pt_bake_dilate(self.h, image.data_ptr(), image.shape[1], image.shape[0], int(passes)))

    def set_probes(self, positions, resolution, columns=None, max_distance=1000.0, enable=True):
        """Light-probe baking (include/mipt.h pt_set_probes): trace() renders an atlas of octahedral maps, resolution x resolution texels
        for each of the K world-space `positions` (K, 3), `columns` probes to an atlas row (default: about a square).  Returns the atlas
        size (W, H) trace() then expects.  The next trace() starts a new accumulation.  Wavefront mode only; not together with set_bake().
        Probes are not part of an accum_save() blob: set the same probes before accum_load().  enable=False returns to the camera."""
        if not enable:
            self._check(self.L.pt_set_probes(self.h, C.byref(abi.PtProbeConfig(0, 0, 0, 0, 0.0)), None))
            return None
        pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        k = len(pos)
        if columns is None:
            columns = max(1, int(np.ceil(np.sqrt(k))))
        cfg = abi.PtProbeConfig(1, int(resolution), k, int(columns), float(max_distance))
        self._check(self.L.pt_set_probes(self.h, C.byref(cfg), _p(pos)))
        return int(columns) * int(resolution), -(-k // int(columns)) * int(resolution)

    def probe_project(self, atlas, kind=0):
        """pt_probe_project: the nine real spherical-harmonic coefficients (bands 0..2) per channel of every probe of a device atlas
        (create_output of the size set_probes() returned): float32 (K, 9, 3).  kind: abi.PROBE_SH_RADIANCE, or abi.PROBE_SH_IRRADIANCE
        for coefficients whose sum over Y_lm(n) is the irradiance on a surface with normal n."""
        # The library writes 27 floats for each probe of ITS layout, which it holds the atlas size to.  A map is at least 16 x 16, so
        # an atlas has at most (W / 16) * (H / 16) cells: room for any layout of this size, however the probes were set.
        cells = max(1, (atlas.shape[1] // 16) * (atlas.shape[0] // 16))
        sh = np.full((cells, 9, 3), np.nan, np.float32)
        self._check(self.L.pt_probe_project(self.h, _dp(atlas), atlas.shape[1], atlas.shape[0], int(kind), _p(sh)))
        written = ~np.isnan(sh).all(axis=(1, 2))                       # the rows the library wrote: its probe count (non-finite texels count as 0)
        return np.ascontiguousarray(sh[:int(np.nonzero(written)[0].max()) + 1 if written.any() else 0])

    def set_matte(self, kind, layers, ids=None):
        """ID mattes (include/mipt.h pt_set_matte): trace() accumulates, beside the output, a ranked list of (id, coverage) pairs per pixel
        in Cryptomatte's layout.  kind: abi.MATTE_INSTANCE or abi.MATTE_MATERIAL; layers: 1 to 4 float32 CUDA tensors (H, W, 4) like the
        output, caller-owned, layer j holding ranks 2j and 2j + 1 (so K = 2 * len(layers)); ids: optional uint32 ids for the first
        len(ids) table rows (the rest get matte_id("instance_<i>") / matte_id("material_<i>")).  layers=None turns mattes off.  The next
        trace() starts a new accumulation.  Wavefront mode only.  The layers are not part of an accum_save() blob: keep them and call
        set_matte() before accum_load().  View a layer's ids with readback(layer).view(np.uint32)[..., 0::2]."""
        if not layers:
            self._check(self.L.pt_set_matte(self.h, C.byref(abi.PtMatteConfig(0, 0, 0, 0)), None))
            self._matte = None
            return
        for t in layers:
            self._image(t)
        idv = None if ids is None else np.ascontiguousarray(ids, np.uint32)
        cfg = abi.PtMatteConfig(1, int(kind), 2 * len(layers), 0 if idv is None else len(idv))
        for j, t in enumerate(layers[:4]):
            cfg.layers[j] = t.data_ptr()
        self._check(self.L.pt_set_matte(self.h, C.byref(cfg), _p(idv) if idv is not None and len(idv) else None))
        self._matte = list(layers)                    # the library keeps the pointers: keep the tensors alive with the renderer

    def motion_snapshot(self, take=True):
        """pt_motion_snapshot: keeps the current pose of every triangle as the previous pose of the frames traced next (builds or refits
        the tree first if it is dirty); take=False frees it.  Pose frame f - 1, call this, pose frame f, trace()."""
        self._check(self.L.pt_motion_snapshot(self.h, int(bool(take))))

    def motion_snapshot_state(self):
        """pt_motion_snapshot_state: abi.MOTION_SNAPSHOT_NONE, _VALID (same rows and triangle counts as when it was taken) or _STALE."""
        out = C.c_int32(-1)
        self._check(self.L.pt_motion_snapshot_state(self.h, C.byref(out)))
        return out.value

    def set_motion(self, motion, prev_world_to_view=None, prev_view_to_clip=None):
        """Motion vectors (include/mipt.h pt_set_motion): trace() accumulates, beside the output, per pixel (previous minus current
        screen position in pixels, previous view depth, current view depth) into `motion`, a float32 CUDA tensor (H, W, 4) like the
        output, caller-owned.  prev_*: the previous frame's camera as 16 floats, glm column-major like PtExecuteParams' (abi.mat4_to_c of
        the camera module's row-major matrices).  motion=None turns the pass off.  The next trace() starts a new accumulation.
        Wavefront mode only, not under a bake or probes.  Neither the target nor the snapshot is part of an accum_save() blob."""
        if motion is None:
            self._check(self.L.pt_set_motion(self.h, C.byref(abi.PtMotionConfig())))
            self._motion = None
            return
        self._image(motion)
        cfg = abi.PtMotionConfig()
        cfg.enable = 1
        cfg.motion = motion.data_ptr()
        cfg.prev_world_to_view[:] = [float(v) for v in np.asarray(prev_world_to_view, np.float32).reshape(-1)]
        cfg.prev_view_to_clip[:] = [float(v) for v in np.asarray(prev_view_to_clip, np.float32).reshape(-1)]
        self._check(self.L.pt_set_motion(self.h, C.byref(cfg)))
        self._motion = motion                         # the library keeps the pointer: keep the tensor alive with the renderer

    def reproject(self, color, motion, prev_color, prev_motion, prev_length=None, out_color=None, out_length=None, config=None):
        """The temporal filter (include/mipt.h pt_reproject): blends `color` with the previous frame's result `prev_color` read at the
        motion vector, where the previous frame's depth (prev_motion.w) agrees.  color / motion / prev_color / prev_motion: float32 CUDA
        tensors (H, W, 4); prev_length: (H, W) float32 history lengths or None (1 everywhere).  out_color: None = a new tensor, `color`
        itself = in place.  config: abi.PtReprojectConfig (None = the defaults).  Asynchronous.  Returns (out_color, out_length)."""
        t = self.torch
        h, w = color.shape[:2]
        if out_color is None:
            out_color = t.empty_like(color)
        if out_length is None:
            out_length = t.empty((h, w), dtype=t.float32, device=color.device)
        for x in (color, motion, prev_color, prev_motion, out_color):
            self._image(x, like=color)
        for x in (prev_length, out_length):
            self._plane(x, h, w, optional=True)
        self._check(self.L.pt_reproject(self.h, _ref(config), _dp(color), _dp(motion), _dp(prev_color), _dp(prev_motion), _dp(prev_length), w, h,
                                        _dp(out_color), _dp(out_length)))
        return out_color, out_length

    def motion_blur(self, color, motion, out=None, config=None):
        """The shutter-time blur along the motion vectors (include/mipt.h pt_motion_blur): a reconstruction filter over `color` and the
        `motion` target of set_motion() (or any images of that layout), both float32 CUDA tensors (H, W, 4).  out: where the result goes
        (None = a new tensor; never an input: there is no in-place mode).  config: abi.PtMotionBlurConfig (None = the defaults).
        Asynchronous on the context's stream.  Returns the output tensor."""
        if out is None:
            out = self.torch.empty_like(color)
        for x in (color, motion, out):
            self._image(x, like=color)
        h, w = color.shape[:2]
        self._check(self.L.pt_motion_blur(self.h, _ref(config), _dp(color), _dp(motion), w, h, _dp(out)))
        return out

    def bloom(self, color, out=None, config=None):
        """The reference's dual-filter bloom over a mip pyramid (include/mipt.h pt_bloom): out = color + strength * the blurred, prefiltered
        `color`, a float32 CUDA tensor (H, W, 4).  out: where the result goes (None = a new tensor; `color` itself filters in place).
        config: abi.PtBloomConfig (None = the defaults).  Asynchronous on the context's stream.  Returns the output tensor."""
        if out is None:
            out = self.torch.empty_like(color)
        for x in (color, out):
            self._image(x, like=color)
        h, w = color.shape[:2]
        self._check(self.L.pt_bloom(self.h, _ref(config), _dp(color), w, h, _dp(out)))
        return out

    def set_variance(self, variance):
        """The variance AOV (include/mipt.h pt_set_variance): trace() keeps, beside the output, per pixel the population variance of the
        samples (rgb per channel, w of the channel sum) in `variance`, a float32 CUDA tensor (H, W, 4) like the output, caller-owned.
        The variance of the pixel's mean is variance / (n - 1).  variance=None turns the pass off.  The next trace() starts a new
        accumulation.  Wavefront mode only.  The target is not part of an accum_save() blob: keep it and call set_variance() before
        accum_load()."""
        if variance is None:
            self._check(self.L.pt_set_variance(self.h, C.byref(abi.PtVarianceConfig())))
            self._variance = None
            return
        self._check(self.L.pt_set_variance(self.h, C.byref(abi.PtVarianceConfig(1, 0, _dp(self._image(variance))))))
        self._variance = variance                     # the library keeps the pointer: keep the tensor alive with the renderer

    def noise_estimate(self, image, variance, samples=0, tile_samples=None, threshold=0.0):
        """The noise report (include/mipt.h pt_noise_estimate): per 16x16 tile the mean and the max of the pixels' relative standard error,
        from the output `image` and the target of set_variance(), both float32 CUDA tensors (H, W, 4).  samples: the count of every tile,
        or tile_samples: (tiles_y, tiles_x) uint32 as adaptive_read() returns them (a tile below 2 reads -1 and is not estimated).
        Returns (tile_mean, tile_max, summary): two (tiles_y, tiles_x) float32 arrays and an abi.PtNoiseSummary whose tiles_above counts
        the tiles whose max exceeds `threshold`.  Synchronises the stream."""
        for x in (image, variance):
            self._image(x, like=image)
        h, w = image.shape[:2]
        ty, tx = _tiles(h, w)
        ts = _tile_samples(tile_samples, h, w)
        mean, mx = np.zeros((ty, tx), np.float32), np.zeros((ty, tx), np.float32)
        summary = abi.PtNoiseSummary()
        self._check(self.L.pt_noise_estimate(self.h, _dp(image), _dp(variance), w, h, _p(ts), int(samples), float(threshold), _p(mean), _p(mx),
                                             C.byref(summary)))
        return mean, mx, summary

    def denoise_variance(self, color, albedo, normal_depth, variance, samples=0, tile_samples=None, out=None, config=None):
        """The a-trous filter steered by the variance AOV (include/mipt.h pt_denoise_variance): color, albedo, normal_depth and variance
        are float32 CUDA tensors (H, W, 4) -- the output of trace() and the targets of set_aov() and set_variance(), or any images of
        those layouts.  samples: the count of every tile, or tile_samples: (tiles_y, tiles_x) uint32 as adaptive_read() returns them (the
        pixels of a tile below 2 come out as they went in).  out: where the result goes (None = a new tensor; `color` itself filters in
        place); config: abi.PtDenoiseVarianceConfig (None = the defaults).  Asynchronous on the context's stream.  Returns the output
        tensor."""
        if out is None:
            out = self.torch.empty_like(color)
        for x in (color, albedo, normal_depth, variance, out):
            self._image(x, like=color)
        h, w = color.shape[:2]
        ts = _tile_samples(tile_samples, h, w)
        self._check(self.L.pt_denoise_variance(self.h, _ref(config), _dp(color), _dp(albedo), _dp(normal_depth), _dp(variance), w, h, _p(ts),
                                               int(samples), _dp(out)))
        return out

    def matte_extract(self, layers, ids, out=None):
        """pt_matte_extract: the anti-aliased mask (H, W) float32 CUDA tensor of a set of 1..64 ids over matte layers (of set_matte(), or
        any tensors of that layout): per pixel the sum of the coverages of the ranks whose id is in the set.  Asynchronous."""
        t = self.torch
        h, w = layers[0].shape[:2]
        if out is None:
            out = t.empty((h, w), dtype=t.float32, device=layers[0].device)
        self._plane(out, h, w)
        ptrs = (C.c_void_p * len(layers))(*[x.data_ptr() for x in layers])
        idv = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        self._check(self.L.pt_matte_extract(self.h, ptrs, 2 * len(layers), w, h, _p(idv), len(idv), _dp(out)))
        return out

    @staticmethod
    def matte_id(name):
        """pt_matte_id: Cryptomatte's 32-bit id of a name (str or bytes).  No GPU call."""
        b = name.encode() if isinstance(name, str) else bytes(name)
        return int(load_library().pt_matte_id(b, len(b)))

    def focus_at(self, settings, params, px, py):
        """Autofocus (include/mipt.h pt_lens_focus_at): the view-space depth of what the pinhole ray through image position (px, py) sees
        (pixel units, pixel centres at + 0.5) -- the focus_distance that puts it in focus -- or None where the ray hits nothing."""
        out = C.c_float()
        rc = self.L.pt_lens_focus_at(self.h, C.byref(settings), C.byref(params), float(px), float(py), C.byref(out))
        if rc == -6:                                  # PT_ERR_NOT_READY: a miss
            return None
        self._check(rc)
        return out.value

    def set_null_shadow_culling(self, on):
        """Skip shadow rays whose contribution is exactly zero (same image, fewer rays than the reference traces)."""
        self._check(self.L.pt_set_null_shadow_culling(self.h, int(bool(on))))

    def set_watertight(self, on):
        """The watertight triangle test (include/mipt.h pt_set_watertight): no ray passes between two triangles that share an edge or a vertex."""
        self._check(self.L.pt_set_watertight(self.h, int(bool(on))))

    def enable_counters(self, on):
        self._check(self.L.pt_enable_counters(self.h, int(on)))

    def set_kernel_mode(self, mode, stage_blocks=0):
        """mode: abi.MODE_WAVEFRONT (default) or abi.MODE_MEGAKERNEL."""
        self._check(self.L.pt_set_kernel_mode(self.h, mode, stage_blocks))

    def build_accel(self):
        """Full build, refit or nothing, whichever the changes since the last call ask for (include/mipt.h pt_build_accel)."""
        self._check(self.L.pt_build_accel(self.h))

    def request_rebuild(self):
        self._check(self.L.pt_accel_request_rebuild(self.h))

    def set_accel_builder(self, builder):
        """abi.BUILDER_LBVH (radix tree), abi.BUILDER_PLOC (clustering by surface area: better tree, slower build) or
        abi.BUILDER_PLOC_REINSERT (the default: the PLOC tree improved by parallel reinsertion passes)."""
        self._check(self.L.pt_set_accel_builder(self.h, int(builder)))

    def enable_stage_timing(self, on):
        self._check(self.L.pt_enable_stage_timing(self.h, int(bool(on))))

    # ---- multi-GPU exchange (RCCL inside libmipt.so; the unique id travels by whatever transport the host has)
    @staticmethod
    def exchange_probe():
        """True if RCCL can be loaded in this process (no GPU call): ranks agree on this before any enters the collective create."""
        return load_library().pt_exchange_probe() == 0

    def exchange_unique_id(self):
        buf = (C.c_ubyte * abi.EXCHANGE_ID_BYTES)()
        rc = self.L.pt_exchange_unique_id(buf)
        if rc != 0:
            raise MiptError("pt_exchange_unique_id failed: %d (RCCL not loadable?)" % rc)
        return bytes(buf)

    def exchange_create(self, rank, world, unique_id=None):
        buf = None if unique_id is None else (C.c_ubyte * abi.EXCHANGE_ID_BYTES).from_buffer_copy(unique_id)
        self._check(self.L.pt_exchange_create(self.h, rank, world, buf))

    def exchange_create_loopback(self, rank, world, group):
        """N contexts of this process exchange by device-to-device copies (no RCCL); call exchange_frame on the root last."""
        self._check(self.L.pt_exchange_create_loopback(self.h, rank, world, C.c_uint64(group)))

    def exchange_frame(self, local, frame=None, mode=abi.EXCHANGE_GATHER, dst=0):
        """local: this rank's accumulation image (H, W, 4) CUDA tensor, only read.  frame: where the root assembles the frame
        (None = in place over the other ranks' tiles of `local`).  Asynchronous on the context's stream."""
        h, w = local.shape[:2]
        self._check(self.L.pt_exchange_frame(self.h, _dp(local), _dp(frame), w, h, mode, dst))

    def exchange_destroy(self):
        self._check(self.L.pt_exchange_destroy(self.h))

    def tiles_packed_bytes(self, width, height, rank, world):
        return int(self.L.pt_tiles_packed_bytes(width, height, rank, world))

    def tiles_pack(self, image, rank, world):
        h, w = image.shape[:2]
        n = self.tiles_packed_bytes(w, h, rank, world) // 16
        packed = self.torch.empty((max(n, 1), 4), dtype=self.torch.float32, device=image.device)
        self._check(self.L.pt_tiles_pack(self.h, _dp(image), w, h, rank, world, _dp(packed)))
        return packed[:n]

    def tiles_unpack(self, packed, image, rank, world):
        h, w = image.shape[:2]
        assert packed.numel() * 4 >= self.tiles_packed_bytes(w, h, rank, world)
        self._check(self.L.pt_tiles_unpack(self.h, _dp(packed), w, h, rank, world, _dp(image)))

    def skin_run(self, params, bones):
        if bones is None or len(bones) == 0:
            self._check(self.L.pt_skin_run(self.h, C.byref(params), None, 0))
        else:
            arr = (abi.PtBone * len(bones))(*bones)
            self._check(self.L.pt_skin_run(self.h, C.byref(params), C.byref(arr), len(bones)))

    # ---- rendering
    def create_output(self, width, height):
        return self.torch.zeros((height, width, 4), dtype=self.torch.float32, device="cuda:%d" % self.device)

    def trace(self, settings, params, output):
        """output: torch float32 CUDA tensor (H, W, 4), the caller-owned accumulation target."""
        assert output.is_cuda and output.is_contiguous() and output.dtype == self.torch.float32
        assert tuple(output.shape) == (params.height, params.width, 4)
        params.output = output.data_ptr()
        self._check(self.L.pt_trace(self.h, C.byref(settings), C.byref(params)))

    def reset_stats(self):
        self._check(self.L.pt_reset_stats(self.h))

    def stats(self):
        s = abi.PtStats()
        self._check(self.L.pt_get_stats(self.h, C.byref(s)))
        return s

    def readback(self, output):
        h, w = output.shape[:2]
        out = np.zeros((h, w, 4), np.float32)
        self._check(self.L.pt_readback(self.h, _dp(output), w, h, _p(out)))
        return out

    def tonemap(self, output, config=None, want_rgba8=False):
        cfg = config or abi.PtTonemapConfig.default()
        h, w = output.shape[:2]
        rgb = np.zeros((h, w, 3), np.float32)
        q = np.zeros((h, w, 4), np.uint8) if want_rgba8 else None
        self._check(self.L.pt_tonemap(self.h, C.byref(cfg), _dp(output), w, h, _p(rgb), _p(q)))
        return (rgb, q) if want_rgba8 else rgb
