"""MK_GUNZIP_REPAIR in the C ABI: the flag's value, the two getters and their binding, and the pinned structs unchanged"""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "metakssd_hip.h")
LIB = os.path.join(ROOT, "metakssd_amd", "lib", "libmetakssd_hip.so")


def test_flag_and_bound():
    src = open(HEADER).read()
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (MK_GUNZIP_(?:MEMBERS|REPAIR|REPAIR_MERGES)) (\d+)u", src)}
    assert vals == {"MK_GUNZIP_MEMBERS": 1, "MK_GUNZIP_REPAIR": 2, "MK_GUNZIP_REPAIR_MERGES": 8}
    from metakssd_amd import capi
    assert (capi.MK_GUNZIP_MEMBERS, capi.MK_GUNZIP_REPAIR, capi.MK_GUNZIP_REPAIR_MERGES) == (1, 2, 8)
    import gunzip_repair_model as rm
    assert rm.MERGES == capi.MK_GUNZIP_REPAIR_MERGES


def test_getters_are_exported_declared_and_bound():
    lib = ctypes.CDLL(LIB)
    src = open(HEADER).read()
    from metakssd_amd import capi
    for name, decl in (("mk_inflate_stream_repairs", "int mk_inflate_stream_repairs(mk_inflate *h, uint64_t *repairs);"),
                       ("mk_sketch_gunzip_repairs", "int mk_sketch_gunzip_repairs(mk_engine *e, uint64_t *repairs);")):
        assert hasattr(lib, name), name
        assert decl in src, name
        assert getattr(capi.lib, name).argtypes == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)], name
    assert capi.lib.mk_inflate_stream_repairs(None, None) == capi.MK_ERR_ARG
    assert capi.lib.mk_sketch_gunzip_repairs(None, None) == capi.MK_ERR_ARG


def test_pinned_structs_did_not_grow():
    from metakssd_amd import capi
    assert (ctypes.sizeof(capi.GunzipOptsC), ctypes.sizeof(capi.GunzipStatsC)) == (16, 104)


def test_binding_keeps_its_call_shapes():
    from metakssd_amd import capi
    for f in (capi.Inflate.stream, capi.Engine.push_gzip, capi.Engine.push_gzip_long, capi.Engine.push_gzip_long_q):
        p = list(inspect.signature(f).parameters.values())
        assert p[-1].name == "repair" and p[-1].default is False, f.__name__  # behind every parameter there was
    # push_gzip_q's parameter list is pinned by tests/test_abi_gunzip_q.py: the -n / -Q entry takes the flag as push_gzip(qmin=, repair=)
    assert "qmin" in inspect.signature(capi.Engine.push_gzip).parameters and "repair" not in inspect.signature(capi.Engine.push_gzip_q).parameters
    assert hasattr(capi.Engine, "gunzip_repairs")


def test_switch_is_in_the_option_loop_and_the_readme():
    """tests/test_cli_surface.py pins the usage text; the switch is documented in the README and in the option loop"""
    assert '"--gunzip-repair")) o->gunzip_opts.flags |= MK_GUNZIP_REPAIR' in open(os.path.join(ROOT, "metakssd_amd", "csrc", "host", "metakssd_main.c")).read()
    assert "--gunzip-repair" in open(os.path.join(ROOT, "README.md")).read()
