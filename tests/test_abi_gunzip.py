"""the many-waves-a-stream gunzip additions to the C ABI: exports, status values and texts, struct sizes"""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "metakssd_hip.h")
LIB = os.path.join(ROOT, "metakssd_amd", "lib", "libmetakssd_hip.so")


def test_new_exports():
    lib = ctypes.CDLL(LIB)
    for name in ("mk_gzip_scan_stream", "mk_inflate_stream", "mk_sketch_push_gzip", "mk_gunzip_pieces_free"):
        assert hasattr(lib, name), name


def test_new_statuses():
    src = open(HEADER).read()
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (MK_INFL_[A-Z_]+) (\d+)", src)}
    assert vals == {"MK_INFL_MISSED": 9, "MK_INFL_CAPACITY": 10}
    from metakssd_amd import capi
    assert (capi.MK_INFL_MISSED, capi.MK_INFL_CAPACITY) == (9, 10)
    texts = {capi.lib.mk_inflate_status_text(s) for s in range(11)}
    assert len(texts) == 11 and b"unknown status" not in texts
    assert capi.lib.mk_inflate_status_text(11) == b"unknown status"


def struct_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), open(HEADER).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        m = re.match(r"\s*(\w+)\s+(.*)", decl.strip(), re.S)
        if m:
            out += [(m.group(1), n.strip().lstrip("*")) for n in m.group(2).split(",")]
    return out


def test_struct_layouts_match_the_binding():
    from metakssd_amd import capi
    size = {"uint32_t": 4, "int32_t": 4, "uint64_t": 8, "int64_t": 8, "double": 8, "mk_gunzip_piece": 8}
    for name, cls, want in (("mk_gunzip_opts", capi.GunzipOptsC, 16), ("mk_gunzip_piece", capi.GunzipPieceC, 16),
                            ("mk_gunzip_pieces", capi.GunzipPiecesC, 16), ("mk_gunzip_stats", capi.GunzipStatsC, 104)):
        fields = struct_fields(name)
        assert [n for _, n in fields] == [n for n, _ in cls._fields_], name
        assert sum(size[t] for t, _ in fields) == ctypes.sizeof(cls) == want, name
