"""tests/composite_model.py is pinned to the reference: on the golden composite cases (marker database and query sketches laid out by the
pinned oracle CLI) its rows, formatted, are the committed composite.tsv that the compiled reference printed.  CPU only."""
import os

import pytest

import composite_model as cm
import golden_cases as gc
import test_golden as tg

shuf_files = tg.shuf_files  # the module-scoped .shuf fixture of the golden tests


@pytest.mark.parametrize("case", ["composite_two_queries_L1K7", "composite_mix_L2K11"])
def test_model_reproduces_reference_golden(case, shuf_files, tmp_path):
    db, qsk = cm.build_marker_db(case, shuf_files, tmp_path, [tg.ORACLE_CLI], [tg.ORACLE_CLI, "set"])
    got = []
    for ln in cm.composite_dirs(db, qsk):
        f = ln.split("\t")
        f[0] = os.path.basename(f[0])
        got.append("\t".join(f))
    want = open(os.path.join(gc.GOLDEN, "expected", case, "composite.tsv")).read().splitlines()
    assert got == want
    assert len(got) == tg.MANIFEST["composite_cases"][case]["lines"] > 0


def test_model_first_occurrence_and_repeats():
    """an id twice in a sample: the first count; an id twice in a reference sketch: two hits"""
    ref = ([10, 11, 12, 13, 14, 14, 20], [0, 6, 7])
    qry = ([14, 10, 11, 12, 13, 14, 20], [9, 1, 2, 3, 4, 500, 7], [0, 7])
    rows = cm.composite_rows(2, [ref], 1, [qry])
    assert rows == [[(0, 6, 1 + 2 + 3 + 4 + 9 + 9, 9, 1, 3, 9)]]


def test_capi_declares_the_composite_entry_points():
    from metakssd_amd import capi
    for name in ("create", "destroy", "load_begin", "load_component", "query_begin", "query_component", "query_finish", "set_option",
                 "last_kernel_ms", "last_counts"):
        fn = getattr(capi.lib, "mk_composite_" + name)
        assert fn.argtypes is not None, name
    assert capi.lib.mk_composite_last_error.restype is not None
    assert capi.COMPOSITE_ROW.itemsize == 28 and capi.COMPOSITE_ROW.names == cm.ROW_FIELDS
    if capi.device_count() == 0:  # no CPU path
        with pytest.raises(capi.MkError) as e:
            capi.Composite(0)
        assert e.value.code == capi.MK_ERR_NO_DEVICE
