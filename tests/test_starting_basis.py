"""CPU: the ABI of ipxk_ipm_starting_basis's two structs, and the seeds of the decision test of
tests/test_gpu_starting_basis.py (its dense restatement alone, no device)."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def kkt():
    from ipx_amd import kkt as k
    return k


def test_struct_layouts(kkt):
    """sizeof and field offsets of ipxk_starting_basis_params / ipxk_starting_basis_info against the ctypes mirrors: the C
    structs hold 8-byte members only, in the header's order"""
    import re
    text = open(os.path.join(ROOT, "include", "ipx_kkt_hip.h")).read()
    for name, mirror in (("ipxk_starting_basis_params", kkt.StartingBasisParams), ("ipxk_starting_basis_info", kkt.StartingBasisInfo)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, text).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                ctype, names = decl.split(None, 1)
                assert ctype in ("ipxint", "double")
                fields += [(nm.strip(), ctype) for nm in names.split(",")]
        assert [f for f, _ in fields] == [f for f, _ in mirror._fields_]
        assert ctypes.sizeof(mirror) == 8 * len(fields)
        for k, (fname, ctype) in enumerate(fields):
            assert getattr(mirror, fname).offset == 8 * k
            assert mirror._fields_[k][1] is (ctypes.c_int64 if ctype == "ipxint" else ctypes.c_double)


def test_decision_seeds_have_margins():
    """every comparison the restatement takes on the decision test's models is decided by a relative margin >= 1e-6, so
    the device's log must equal it exactly"""
    import test_gpu_starting_basis as T
    for seed, m, n in T.DECISION_CASES[:1]:
        P = T.general_lp(m, n, seed, dep=2)
        it0, _ = T.random_iterate(P, seed + 100)
        R = T.restatement(P, it0)
        assert R["margin"] >= 1e-6 and len(R["dep_cols"]) == 2 and len(R["dep_rows"]) == 2
        assert R["cols_inconsistent"] == 0 and R["rows_inconsistent"] == 0
