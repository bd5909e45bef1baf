"""The snapshot file format of include/dsr_snapshot.h in pure numpy: `read_snapshot(path) -> dict of arrays`, `write_snapshot`.

For tests and tooling: no library, no GPU.  `read_snapshot` validates what the C loader validates at header level (magic, version,
table, length) and every section's checksum, and raises `SnapshotFormatError` naming the cause.  The arrays come back in the
layouts the engine's `dump_*` calls use, so that a saved file can be compared with them bit for bit; `raw=True` returns the sections
as byte arrays instead (what `write_snapshot` takes)."""
import struct

import numpy as np

MAGIC = b"DSRSNAP\0"
FORMAT_VERSION = 1
HEADER_BYTES = 128
TABLE_ENTRY_BYTES = 32
BLOCK_PAYLOAD_BYTES = 3584
ALIGN = 64
PARAMS_BYTES = 192
CTR_COUNT, WORK_COUNT = 32, 8

# section ids (enum dsr_snapshot_section)
SECTIONS = {
    "params": 1, "hash_table": 2, "voxel_alloc_list": 3, "excess_alloc_list": 4, "counters": 5, "block_ids": 6, "block_payload": 7,
    "visible_ids": 8, "visible_blocks": 9, "visible_types": 10, "range_image": 11, "raycast_result": 12, "raycast_image": 13,
    "ray_box": 14, "icp_points": 15, "icp_normals": 16, "icp_pose": 17, "view_rgba": 18, "view_depth": 19, "view_raw_depth": 20,
    "gc_fifo": 21, "swap_state": 22, "swap_stored": 23, "swap_slot": 24, "host_blocks": 25, "free_visible_ids": 26,
    "free_visible_blocks": 27, "free_range_image": 28, "free_raycast_result": 29, "free_raycast_image": 30, "free_ray_box": 31,
}
SECTION_NAMES = {v: k for k, v in SECTIONS.items()}

HASH_ENTRY_DTYPE = np.dtype([("pos", "<i2", (3,)), ("pad", "<i2"), ("offset", "<i4"), ("ptr", "<i4")])
VOXEL_DTYPE = np.dtype([("sdf", "<i2"), ("w_depth", "u1"), ("clr", "u1", (3,)), ("w_color", "u1"), ("pad", "u1")])
PARAMS_DTYPE = np.dtype([("m", "<f4", (16,)), ("inv_m", "<f4", (16,)), ("depth_weighting", "<i4"), ("has_view", "<i4"),
                         ("frames_processed", "<i8"), ("fifo_len", "<i4"), ("fifo_cap", "<i4"), ("view_box", "<i4", (4,)),
                         ("host_slots", "<i4"), ("reserved", "<i4", (5,))])
assert HASH_ENTRY_DTYPE.itemsize == 16 and VOXEL_DTYPE.itemsize == 8 and PARAMS_DTYPE.itemsize == PARAMS_BYTES

_SETTINGS = ("voxel_size", "mu", "max_w", "hash_bucket_num", "excess_list_size", "sdf_local_block_num", "width", "height",
             "rgb_width", "rgb_height", "use_swapping", "depth_weighting")
_SETTINGS_FMT = "<ffiiiiiiiiii"


class SnapshotFormatError(ValueError):
    pass


def checksum(data):
    """The section checksum of dsr_snapshot.h over `data` (bytes or a uint8 array)."""
    b = np.frombuffer(bytes(data) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).view(np.uint8).tobytes(), np.uint8)
    if len(b) % 4:
        b = np.concatenate([b, np.zeros(4 - len(b) % 4, np.uint8)])
    w = b.view("<u4").astype(np.uint64)
    n = len(w)
    with np.errstate(over="ignore"):
        a = np.add.reduce(w, dtype=np.uint64) if n else np.uint64(0)
        bb = np.add.reduce(np.arange(n, 0, -1, dtype=np.uint64) * w, dtype=np.uint64) if n else np.uint64(0)
        return int((np.uint64(a) + np.uint64(bb) * np.uint64(0x9E3779B97F4A7C15)) & np.uint64(0xFFFFFFFFFFFFFFFF))


def _align(v):
    return (v + ALIGN - 1) // ALIGN * ALIGN


def read_header(buf):
    """-> (settings dict, [(id, offset, bytes, checksum)]) of the snapshot whose bytes are `buf`; SnapshotFormatError otherwise."""
    total = len(buf)
    if total < HEADER_BYTES:
        raise SnapshotFormatError("short file (no complete header)")
    if bytes(buf[:8]) != MAGIC:
        raise SnapshotFormatError("bad magic (not a snapshot file)")
    version, header_bytes = struct.unpack_from("<II", buf, 8)
    if version != FORMAT_VERSION:
        raise SnapshotFormatError(f"bad version (format {version}, this reader reads {FORMAT_VERSION})")
    if header_bytes != HEADER_BYTES:
        raise SnapshotFormatError("bad header size")
    info = dict(zip(_SETTINGS, struct.unpack_from(_SETTINGS_FMT, buf, 16)))
    info["owned_blocks"], info["file_bytes"] = struct.unpack_from("<QQ", buf, 64)
    n, mask = struct.unpack_from("<II", buf, 80)
    info["section_mask"] = mask
    if n == 0 or n > 32:
        raise SnapshotFormatError("malformed section table (count)")
    need = HEADER_BYTES + n * TABLE_ENTRY_BYTES
    if total < need:
        raise SnapshotFormatError("short file (truncated section table)")
    if info["file_bytes"] != total:
        raise SnapshotFormatError(f"short file ({total} of {info['file_bytes']} bytes)" if total < info["file_bytes"]
                                  else "file longer than its header says")
    table, end, seen = [], need, 0
    for i in range(n):
        sid, _, off, nbytes, csum = struct.unpack_from("<IIQQQ", buf, HEADER_BYTES + i * TABLE_ENTRY_BYTES)
        if sid == 0 or sid >= 32 or seen & (1 << sid):
            raise SnapshotFormatError("malformed section table (id)")
        if off % ALIGN or off < end or off > total or nbytes > total - off:
            raise SnapshotFormatError(f"malformed section table (section {sid} outside the file)")
        end = off + nbytes
        seen |= 1 << sid
        table.append((sid, off, nbytes, csum))
    if seen != mask:
        raise SnapshotFormatError("malformed section table (mask)")
    return info, table


def _typed(name, raw, info):
    H, W = info["height"], info["width"]
    mh, mw = (H + 7) // 8, (W + 7) // 8
    if name == "params":
        return raw.view(PARAMS_DTYPE)[0]
    if name == "hash_table":
        return raw.view(HASH_ENTRY_DTYPE)
    if name in ("voxel_alloc_list", "excess_alloc_list", "block_ids", "visible_ids", "free_visible_ids", "swap_slot", "ray_box", "free_ray_box"):
        return raw.view("<i4")
    if name in ("visible_blocks", "free_visible_blocks"):
        return raw.view("<i4").reshape(-1, 4)
    if name in ("range_image", "free_range_image"):
        return raw.view("<f4").reshape(mh, mw, 2)
    if name in ("raycast_result", "free_raycast_result", "icp_points", "icp_normals"):
        return raw.view("<f4").reshape(H, W, 4)
    if name in ("raycast_image", "free_raycast_image"):
        return raw.reshape(H, W, 4)
    if name == "view_rgba":
        return raw.reshape(info["rgb_height"], info["rgb_width"], 4)
    if name == "view_depth":
        return raw.view("<f4").reshape(H, W)
    if name == "view_raw_depth":
        return raw.view("<i2").reshape(H, W)
    if name == "icp_pose":
        return raw.view("<f4")
    if name == "gc_fifo":
        return raw.view("<u4").reshape(-1, (info["hash_bucket_num"] + info["excess_list_size"] + 31) // 32) if len(raw) else raw.view("<u4")
    if name == "host_blocks":
        return raw.reshape(-1, 4096)
    return raw


def payload_to_voxels(payload):
    """BLOCK_PAYLOAD (n x 3584 bytes) -> n x 512 voxels in the layout of dump_voxel_blocks."""
    p = np.ascontiguousarray(payload).reshape(-1, BLOCK_PAYLOAD_BYTES)
    out = np.zeros((len(p), 512), VOXEL_DTYPE)
    out["sdf"] = p[:, :1024].copy().view("<i2")
    out["w_depth"] = p[:, 1024:1536]
    clr = p[:, 1536:].reshape(-1, 512, 4)
    out["clr"] = clr[:, :, :3]
    out["w_color"] = clr[:, :, 3]
    return out


def host_block_to_voxels(block):
    """One 4096-byte block of HOST_BLOCKS -> 512 voxels in the layout of dump_stored_block."""
    b = np.ascontiguousarray(block).reshape(4096)
    return payload_to_voxels(np.concatenate([b[:1536], b[2048:]]))[0]


def read_snapshot(path, raw=False):
    """-> dict: the header's settings under "info", every section under its name (SECTIONS), "counters" split into "ctr" (32 x int32)
    and "work" (8 x uint64), and "voxels": the payload as n x 512 voxels.  Raises SnapshotFormatError."""
    with open(path, "rb") as f:
        buf = f.read()
    info, table = read_header(buf)
    out = {"info": info}
    for sid, off, nbytes, csum in table:
        data = np.frombuffer(buf, np.uint8, nbytes, off).copy()
        if checksum(data) != csum:
            raise SnapshotFormatError(f"checksum mismatch in section {sid}")
        name = SECTION_NAMES.get(sid, f"section_{sid}")
        out[name] = data if raw else _typed(name, data, info)
    if not raw:
        if "counters" in out:
            c = out["counters"]
            out["ctr"] = c[:CTR_COUNT * 4].view("<i4")
            out["work"] = c[CTR_COUNT * 4:].view("<u8")
        if "block_payload" in out:
            out["voxels"] = payload_to_voxels(out["block_payload"])
    return out


def write_snapshot(path, info, sections):
    """Write a snapshot file: `info` holds the header's settings (the keys of read_snapshot's "info"; "owned_blocks" defaults to the
    payload's block count), `sections` maps names or ids to arrays (their bytes are written as they are), in ascending id order."""
    items = sorted(((SECTIONS[k] if isinstance(k, str) else int(k)), np.ascontiguousarray(v).view(np.uint8).reshape(-1)) for k, v in sections.items())
    if not items:
        raise ValueError("a snapshot has at least one section")
    off = HEADER_BYTES + len(items) * TABLE_ENTRY_BYTES
    table = []
    for sid, data in items:
        start = _align(off)
        table.append((sid, start, len(data), checksum(data)))
        off = start + len(data)
    total = off
    buf = bytearray(total)
    buf[:8] = MAGIC
    struct.pack_into("<II", buf, 8, FORMAT_VERSION, HEADER_BYTES)
    struct.pack_into(_SETTINGS_FMT, buf, 16, *[info.get(k, 0) for k in _SETTINGS])
    owned = info.get("owned_blocks")
    if owned is None:
        owned = next((len(d) // BLOCK_PAYLOAD_BYTES for sid, d in items if sid == SECTIONS["block_payload"]), 0)
    struct.pack_into("<QQ", buf, 64, owned, total)
    mask = 0
    for sid, *_ in table:
        mask |= 1 << sid
    struct.pack_into("<II", buf, 80, len(items), mask)
    for i, ((sid, start, n, csum), (_, data)) in enumerate(zip(table, items)):
        struct.pack_into("<IIQQQ", buf, HEADER_BYTES + i * TABLE_ENTRY_BYTES, sid, 0, start, n, csum)
        buf[start:start + n] = data.tobytes()
    with open(path, "wb") as f:
        f.write(buf)
    return total
