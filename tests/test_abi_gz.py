"""the gzip additions to the C ABI: the new exports exist, the inflate statuses kept their values"""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "metakssd_hip.h")
LIB = os.path.join(ROOT, "metakssd_amd", "lib", "libmetakssd_hip.so")


def test_new_exports():
    lib = ctypes.CDLL(LIB)
    for name in ("mk_gzip_scan", "mk_inflate_members", "mk_sketch_batch_begin_gz", "mk_sketch_batch_gz_status"):
        assert hasattr(lib, name), name


def test_inflate_statuses_keep_their_values():
    src = open(HEADER).read()
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(MK_INFL_[A-Z_]+) = (\d+)", src)}
    assert vals == {"MK_INFL_OK": 0, "MK_INFL_BAD_BLOCK": 1, "MK_INFL_BAD_LENGTHS": 2, "MK_INFL_BAD_CODE": 3, "MK_INFL_BAD_DISTANCE": 4,
                    "MK_INFL_INPUT": 5, "MK_INFL_OUTPUT_LEN": 6, "MK_INFL_CRC": 7, "MK_INFL_TRAILING": 8}
    from metakssd_amd import capi
    assert (capi.MK_INFL_CRC, capi.MK_INFL_TRAILING) == (7, 8)
    assert capi.lib.mk_inflate_status_text(8) not in (None, b"unknown status")
    assert capi.lib.mk_inflate_status_text(7) == b"CRC mismatch"
    assert int(re.search(r"#define MK_CRC_SLICE (\d+)u", src).group(1)) == capi.MK_CRC_SLICE
