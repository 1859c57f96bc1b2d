"""The checkpoint file format (include/immesh_checkpoint.h) restated in numpy: header, section table, checksum, a reader, a writer, and a builder
of small valid and invalid files for the tests that need no device.  Nothing here calls the library."""
import numpy as np

from immesh_amd import capi

MAGIC = b"IMMESHCK"
VERSION = 1
ALIGN = 64
GOLDEN = np.uint64(0x9E3779B97F4A7C15)

# record sizes and strides a file carries (CkFileHeader::rec), in file order
REC = (("sizeof(NodeRec)", 384), ("sizeof(HashEnt)", 16), ("sizeof(MeshGridEnt)", 32), ("sizeof(MeshVoxEnt)", 16), ("sizeof(RgEnt)", 16), ("MV_VOX_CAP", 128),
       ("MV_ADJ_STRIDE", 16), ("IM_CHUNK_PTS", 16), ("IM_PT_DOUBLES", 9), ("IM_EXT_CHUNKS", 2048), ("leaf chunk words", 16), ("sizeof(immesh_counters_t)", 176),
       ("SC_COUNT", 24), ("PC_COUNT", 8), ("MESH_NPAR", 3), ("STATS_WORDS", 16 + 64 * 16))
COUNTS = ("roots", "nodes", "chunks", "free_ready", "free_pending", "ext", "leaf", "verts", "voxels", "tris", "live", "adj", "regions", "scans_meshed",
          "map_updates", "mesh_jobs")
HOST_STATE_BYTES = 176 + 24 * 8 + 16 + 16

CONFIG_DTYPE = np.dtype(capi.Config)
HEADER_DTYPE = np.dtype([("magic", "S8"), ("version", "<i4"), ("header_bytes", "<i4"), ("n_sections", "<i4"), ("section_bytes", "<i4"), ("file_bytes", "<i8"),
                         ("payload_offset", "<i8"), ("header_checksum", "<u8"), ("has_regions", "<i4"), ("has_colour", "<i4"), ("rec", "<i4", 16), ("masks", "<u8", 4),
                         ("counts", "<i8", 16), ("cfg", "V288")])   # cfg: the raw bytes of an immesh_config (CONFIG_DTYPE), padding included
SECTION_DTYPE = np.dtype([("name", "S24"), ("offset", "<i8"), ("bytes", "<i8"), ("records", "<i8"), ("checksum", "<u8")])
assert HEADER_DTYPE.itemsize == 568 and SECTION_DTYPE.itemsize == 56 and CONFIG_DTYPE.itemsize == 288


def mix64(k):
    """the splitmix64 finaliser on uint64 arrays (wrapping arithmetic)"""
    k = np.asarray(k, np.uint64).copy()
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(30); k *= np.uint64(0xbf58476d1ce4e5b9)
        k ^= k >> np.uint64(27); k *= np.uint64(0x94d049bb133111eb)
        k ^= k >> np.uint64(31)
    return k


def checksum(data, first_word=0):
    """sum over the 8-byte words w_i of `data` (tail zero-padded) of mix64(w_i ^ ((first_word + i) * 0x9E3779B97F4A7C15)) mod 2^64"""
    raw = np.frombuffer(bytes(data) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).tobytes(), np.uint8)
    pad = (-len(raw)) % 8
    words = np.concatenate([raw, np.zeros(pad, np.uint8)]).view("<u8")
    with np.errstate(over="ignore"):
        idx = (np.arange(len(words), dtype=np.uint64) + np.uint64(first_word)) * GOLDEN
        return int(mix64(words ^ idx).sum(dtype=np.uint64))


def layout(counts, tables, has_regions=False, has_colour=False):
    """[(name, bytes per record, records)] of a file, in file order.  counts: dict over COUNTS; tables: occupied slots of
    (reg.hash, mesh.grid, mesh.vox, mesh.thash, rg.hash)"""
    n = counts
    out = []

    def table(base, ent, k):
        out.extend([(base + ".slot", 4, tables[k]), (base + ".ent", ent, tables[k])])

    out += [("reg.counters", 4, 16), ("reg.stats", 8, 16 + 64 * 16)]
    table("reg.hash", 16, 0)
    out += [("reg.nodes", 384, n["nodes"]), ("reg.chunks", 16 * 9 * 8, n["chunks"]), ("reg.ext", 2048 * 4, n["ext"]), ("reg.leaf", 64, n["leaf"]),
            ("reg.free_ready", 4, n["free_ready"]), ("reg.free_pending", 4, n["free_pending"]),
            ("mesh.pc", 4, 8), ("mesh.v_pos", 12, n["verts"]), ("mesh.v_smooth", 24, n["verts"]), ("mesh.v_voxel", 4, n["verts"])]
    table("mesh.grid", 32, 1)
    table("mesh.vox", 16, 2)
    out += [("mesh.vx_key", 8, n["voxels"]), ("mesh.vx_npts", 4, n["voxels"]), ("mesh.vx_pts", 128 * 4, n["voxels"]), ("mesh.vx_meshing_times", 4, n["voxels"]),
            ("mesh.vx_new_added", 4, n["voxels"]), ("mesh.vx_stamp", 4, n["voxels"])]
    out += [("mesh.vx_rank_seq%d" % p, 4, n["voxels"]) for p in range(3)]
    out += [("mesh.vx_short_axis", 24, n["voxels"]), ("mesh.t_v", 12, n["tris"]), ("mesh.t_word", 8, n["tris"]), ("mesh.t_live", 4, n["tris"]),
            ("mesh.t_rem_seq", 4, n["tris"]), ("mesh.t_flip", 1, n["tris"])]
    table("mesh.thash", 4, 3)
    out += [("mesh.a_head", 4, n["verts"]), ("mesh.a_chunks", 64, n["adj"]), ("host.state", HOST_STATE_BYTES, 1)]
    if has_regions:
        out += [("rg.cnt", 4, 8)]
        table("rg.hash", 16, 4)
        out += [("rg.r_key", 12, n["regions"]), ("rg.r_nlive", 4, n["regions"]), ("rg.r_dirty", 4, n["regions"]), ("rg.t_region", 4, n["tris"])]
    if has_colour:
        out += [("cl.rgb%d" % k, 8, n["verts"]) for k in range(3)] + [("cl.cov%d" % k, 8, n["verts"]) for k in range(3)]
        out += [("cl.first_exposure", 8, n["verts"]), ("cl.obs_dis", 8, n["verts"]), ("cl.last_obs_time", 8, n["verts"]), ("cl.n_obs", 4, n["verts"])]
    return out


def header_checksum(header, table):
    raw = bytearray(header.tobytes())
    raw[40:48] = bytes(8)   # the header_checksum field itself counts as zero
    return (checksum(bytes(raw)) + checksum(table.tobytes(), HEADER_DTYPE.itemsize // 8)) & ((1 << 64) - 1)


def assemble(header, table, payloads):
    """file bytes from a header record, a section table and the sections' payload bytes (placed at the table's offsets, gaps zero)"""
    size = int(header["file_bytes"])
    buf = bytearray(max(size, int(header["payload_offset"])))
    for sec, data in zip(table, payloads):
        o = int(sec["offset"])
        data = data[:max(0, len(buf) - o)]   # (a table that points past the end: the file keeps its length)
        buf[o:o + len(data)] = data
    buf[:HEADER_DTYPE.itemsize] = header.tobytes()
    buf[HEADER_DTYPE.itemsize:HEADER_DTYPE.itemsize + table.nbytes] = table.tobytes()
    return bytes(buf)


def build(cfg=None, counts=None, tables=(3, 2, 2, 5, 1), has_regions=False, has_colour=False, seed=0):
    """a small valid checkpoint -> (header record, section table, [payload bytes]); the payload is random bytes of the right sizes"""
    rng = np.random.default_rng(seed)
    n = dict(roots=3, nodes=4, chunks=5, free_ready=2, free_pending=0, ext=1, leaf=2, verts=7, voxels=2, tris=5, live=4, adj=3, regions=1 if has_regions else 0,
             scans_meshed=2, map_updates=2, mesh_jobs=2)
    n.update(counts or {})
    specs = layout(n, tables, has_regions, has_colour)
    header = np.zeros((), HEADER_DTYPE)
    header["magic"] = MAGIC; header["version"] = VERSION; header["header_bytes"] = HEADER_DTYPE.itemsize; header["section_bytes"] = SECTION_DTYPE.itemsize
    header["n_sections"] = len(specs); header["has_regions"] = int(has_regions); header["has_colour"] = int(has_colour)
    header["rec"] = [v for _, v in REC]
    header["masks"] = [(1 << 17) - 1, (1 << 19) - 1, (1 << 19) - 1, (1 << 21) - 1]
    header["counts"] = [n[k] for k in COUNTS]
    header["cfg"] = np.void(bytes(cfg if cfg is not None else capi.avia_config()))
    table = np.zeros(len(specs), SECTION_DTYPE)
    payload_offset = -(-(HEADER_DTYPE.itemsize + table.nbytes) // ALIGN) * ALIGN
    payloads, off = [], payload_offset
    for i, (name, elem, records) in enumerate(specs):
        data = rng.integers(0, 256, elem * records, dtype=np.uint8).tobytes()
        payloads.append(data)
        table[i] = (name.encode(), off, len(data), records, checksum(data))
        off = -(-(off + len(data)) // ALIGN) * ALIGN
    header["payload_offset"] = payload_offset; header["file_bytes"] = off
    header["header_checksum"] = header_checksum(header, table)
    return header, table, payloads


def read(path):
    """-> (header record, section table, {name: payload bytes}); asserts what a reader must check"""
    raw = open(path, "rb").read()
    header = np.frombuffer(raw[:HEADER_DTYPE.itemsize], HEADER_DTYPE)[0]
    assert header["magic"] == MAGIC and header["version"] == VERSION and header["file_bytes"] == len(raw)
    assert list(header["rec"]) == [v for _, v in REC]
    ns = int(header["n_sections"])
    table = np.frombuffer(raw[HEADER_DTYPE.itemsize:HEADER_DTYPE.itemsize + ns * SECTION_DTYPE.itemsize], SECTION_DTYPE)
    assert header_checksum(header, table) == int(header["header_checksum"])
    out = {}
    for sec in table:
        data = raw[int(sec["offset"]):int(sec["offset"]) + int(sec["bytes"])]
        assert checksum(data) == int(sec["checksum"]), sec["name"]
        out[sec["name"].decode()] = data
    return header, table, out
