"""The batch entry points of the covariance and residual libraries without a device: the headers, the ctypes layouts that mirror
them, the exports, and the calls that return before touching a device (an empty batch, a negative count)."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

INC = os.path.join(ROOT, "include")


def struct_fields(header, name):
    """Field names of `typedef struct name { ... } name;` in declaration order."""
    src = open(os.path.join(INC, header)).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            out += [re.sub(r"[^\w]", "", part.split()[-1]) for part in decl.split(",")]
    return out


def test_versions_are_bumped(vio):
    assert "#define VIO_COV_VERSION 2" in open(os.path.join(INC, "vio_covariance.h")).read()
    assert "#define VIO_RES_VERSION 2" in open(os.path.join(INC, "vio_residuals.h")).read()
    assert vio.CovLib(vio.COV_LIB).fn["version"]() == 2
    assert vio.ResLib(vio.RES_LIB).fn["version"]() == 2


def test_ctypes_items_mirror_the_headers(vio):
    cov = [f for f, _ in vio.covariance.VioCovBatchItem._fields_]
    res = [f for f, _ in vio.residuals.VioResBatchItem._fields_]
    assert cov == struct_fields("vio_covariance.h", "vio_cov_batch_item")
    assert res == struct_fields("vio_residuals.h", "vio_res_batch_item")
    assert C.sizeof(vio.covariance.VioCovBatchItem) == 9 * 8
    assert C.sizeof(vio.residuals.VioResBatchItem) == 12 * 8


def test_batch_entry_points_are_exported(vio):
    for path, sym in ((vio.COV_LIB, "vio_cov_compute_batch"), (vio.RES_LIB, "vio_res_compute_batch")):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert re.search(r"\bT %s\b" % sym, out), sym


def test_empty_and_negative_batches(vio):
    cov, res = vio.CovLib(vio.COV_LIB), vio.ResLib(vio.RES_LIB)
    assert cov.fn["compute_batch"](None, 0, 1, 0, None, None) == 0          # VIO_OK: nothing to do
    assert res.fn["compute_batch"](None, 0, 0, None, 1.0, 3.0) == 0
    assert cov.fn["compute_batch"](None, -1, 1, 0, None, None) == -1        # VIO_ERR_BAD_ARG
    assert res.fn["compute_batch"](None, -1, 0, None, 1.0, 3.0) == -1
    assert cov.fn["compute_batch"](None, 2, 1, 0, None, None) == -1         # NULL handle array
    assert res.fn["compute_batch"](None, 2, 0, None, 1.0, 3.0) == -1
