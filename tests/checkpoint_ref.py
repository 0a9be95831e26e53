"""Independent writer and parser of the accumulation checkpoint blob (include/mipt.h, the comment above pt_accum_save): struct, zlib.crc32
and a numpy tile pack.  Written from the header's field table, not from the C++; tests/test_checkpoint_host.py feeds its blobs to
pt_accum_inspect and tests/test_gpu_checkpoint.py parses pt_accum_save's blobs with it.

  rank_tiles     the global ids of a rank's 16x16 tiles, in the rank's local order
  pack / unpack  pt_tiles_pack's layout: 256 float4 per tile, one 8x8 quadrant after the other (quadrants row-major, pixels row-major
                 within a quadrant), pixels outside the image as zeros
  write / parse  the 160-byte header and the sections after it
"""
import struct
import zlib

import numpy as np

f32 = np.float32
TILE = 16
MAGIC = b"MIPTACC1"
HEADER = "<8sIIQIIIIIIiIQ16f3if4I"          # little-endian, no padding: 160 bytes
HEADER_BYTES = 160
OUTPUT, ALBEDO, NORMAL_DEPTH, ADAPTIVE = 1, 2, 4, 8
IMAGE_KEYS = ("output", "albedo", "normal_depth")
assert struct.calcsize(HEADER) == HEADER_BYTES


def tile_grid(width, height):
    return (width + TILE - 1) // TILE, (height + TILE - 1) // TILE


def rank_tiles(width, height, rank=0, world=1):
    tx, ty = tile_grid(width, height)
    return list(range(rank, tx * ty, world))


def packed_bytes(width, height, rank=0, world=1):
    return len(rank_tiles(width, height, rank, world)) * 256 * 16


def _slot_offsets():
    t = np.arange(256)
    quad, lane = t >> 6, t & 63
    return (quad >> 1) * 8 + (lane >> 3), (quad & 1) * 8 + (lane & 7)       # dy, dx within the tile


def pack(image, rank=0, world=1):
    """(H, W, 4) float32 -> (tiles * 256, 4) float32 of the rank's tiles."""
    image = np.asarray(image, f32)
    h, w = image.shape[:2]
    tx, _ = tile_grid(w, h)
    tiles = rank_tiles(w, h, rank, world)
    dy, dx = _slot_offsets()
    out = np.zeros((len(tiles), 256, 4), f32)
    for k, t in enumerate(tiles):
        y, x = (t // tx) * TILE + dy, (t % tx) * TILE + dx
        ok = (y < h) & (x < w)
        out[k, ok] = image[y[ok], x[ok]]
    return out.reshape(-1, 4)


def unpack(packed, image, rank=0, world=1):
    """Writes the rank's tiles of `image` (H, W, 4) from `packed`; other pixels stay."""
    h, w = image.shape[:2]
    tx, _ = tile_grid(w, h)
    tiles = rank_tiles(w, h, rank, world)
    dy, dx = _slot_offsets()
    p = np.asarray(packed, f32).reshape(len(tiles), 256, 4)
    for k, t in enumerate(tiles):
        y, x = (t // tx) * TILE + dy, (t % tx) * TILE + dx
        ok = (y < h) & (x < w)
        image[y[ok], x[ok]] = p[k, ok]
    return image


def seal(blob):
    """Stores zlib.crc32 of bytes [28, end) at offset 24."""
    b = bytearray(blob)
    b[24:28] = struct.pack("<I", zlib.crc32(bytes(b[28:])) & 0xffffffff)
    return bytes(b)


def write(width, height, accumulated_frames, output, albedo=None, normal_depth=None, adaptive=None, rank=0, world=1, next_frame=0,
          world_to_clip=None):
    """adaptive = dict(config=(enable, min_samples, max_samples, threshold), active=, samples=, error= (one entry per tile of the rank, in
    its local order), half=(H, W, 4)) or None."""
    tiles = len(rank_tiles(width, height, rank, world))
    images = [output, albedo, normal_depth]
    sections = sum(1 << k for k, im in enumerate(images) if im is not None) | (ADAPTIVE if adaptive else 0)
    payload = b"".join(pack(im, rank, world).tobytes() for im in images if im is not None)
    cfg = (0, 0, 0, 0.0)
    if adaptive:
        cfg = adaptive["config"]
        rec = np.zeros((tiles, 4), np.uint32)
        rec[:, 0] = np.asarray(adaptive["active"], np.uint32)
        rec[:, 1] = np.asarray(adaptive["samples"], np.uint32)
        rec[:, 2] = np.asarray(adaptive["error"], f32).view(np.uint32)
        payload += rec.tobytes() + pack(adaptive["half"], rank, world).tobytes()
    total = HEADER_BYTES + len(payload)
    w2c = [0.0] * 16 if world_to_clip is None else [float(x) for x in np.asarray(world_to_clip, f32).ravel()]
    head = struct.pack(HEADER, MAGIC, 1, HEADER_BYTES, total, 0, sections, width, height, rank, world, accumulated_frames, tiles,
                       next_frame, *w2c, int(cfg[0]), int(cfg[1]), int(cfg[2]), float(cfg[3]), 0, 0, 0, 0)
    return seal(head + payload)


def parse(blob):
    """The header's fields and the sections as arrays; asserts the framing (magic, sizes, crc)."""
    blob = bytes(blob)
    assert len(blob) >= HEADER_BYTES
    v = struct.unpack(HEADER, blob[:HEADER_BYTES])
    d = dict(magic=v[0], version=v[1], header_bytes=v[2], total_bytes=v[3], crc32=v[4], sections=v[5], width=v[6], height=v[7],
             tile_rank=v[8], tile_rank_count=v[9], accumulated_frames=v[10], tiles=v[11], next_frame=v[12],
             world_to_clip=np.array(v[13:29], f32), adaptive=(v[29], v[30], v[31], v[32]), reserved=v[33:37])
    assert d["magic"] == MAGIC and d["version"] == 1 and d["header_bytes"] == HEADER_BYTES and d["total_bytes"] == len(blob)
    assert d["crc32"] == zlib.crc32(blob[28:]) & 0xffffffff
    assert d["tiles"] == len(rank_tiles(d["width"], d["height"], d["tile_rank"], d["tile_rank_count"]))
    P, at = d["tiles"] * 256 * 16, HEADER_BYTES
    for k, key in enumerate(IMAGE_KEYS):
        d[key] = None
        if d["sections"] & (1 << k):
            d[key] = np.frombuffer(blob, f32, P // 4, at).reshape(-1, 4)
            at += P
    d["records"] = d["half"] = None
    if d["sections"] & ADAPTIVE:
        d["records"] = np.frombuffer(blob, np.uint32, d["tiles"] * 4, at).reshape(-1, 4)
        at += d["tiles"] * 16
        d["half"] = np.frombuffer(blob, f32, P // 4, at).reshape(-1, 4)
        at += P
    assert at == len(blob)
    return d
