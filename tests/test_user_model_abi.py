"""CPU: the structs of the header's "user model" section against their ctypes declarations (field order, offsets, sizes, as
the C compiler lays them out), and the example program against the header."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ipx_kkt_hip.h")
STRUCTS = {"ipxk_lp_params": "LpParams", "ipxk_lp_info": "LpInfo", "ipxk_lp_eval": "LpEval"}
CTYPES = {"ipxint": ctypes.c_int64, "double": ctypes.c_double, "int": ctypes.c_int}


def header_fields(name):
    """[(type, field)] of `typedef struct name { ... } name;` in declaration order"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), text, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            out += [(ctype, f.strip()) for f in names.split(",")]
    return out


@pytest.mark.parametrize("cname", sorted(STRUCTS))
def test_struct_fields_match_ctypes(cname):
    from ipx_amd import kkt
    S = getattr(kkt, STRUCTS[cname])
    fields = header_fields(cname)
    assert [f for _, f in fields] == [f for f, _ in S._fields_]
    assert [CTYPES[t] for t, _ in fields] == [t for _, t in S._fields_]


def test_struct_layout_matches_compiler(tmp_path):
    from ipx_amd import kkt
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "ipx_kkt_hip.h"', "int main() {"]
    for cname in sorted(STRUCTS):
        lines.append('    std::printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for _, f in header_fields(cname):
            lines.append('    std::printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines.append("}")
    src = tmp_path / "layout.cc"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call([cxx, "-std=c++14", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(ln.split() for ln in subprocess.check_output([exe], text=True).splitlines())
    for cname, pyname in STRUCTS.items():
        S = getattr(kkt, pyname)
        assert int(got[cname]) == ctypes.sizeof(S), cname
        for f, _ in S._fields_:
            assert int(got["%s.%s" % (cname, f)]) == getattr(S, f).offset, (cname, f)


def test_example_compiles_against_header():
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    subprocess.check_call([cxx, "-std=c++14", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "lp_user.cc")])


def test_makefile_builds_the_example():
    text = open(os.path.join(ROOT, "examples", "Makefile")).read()
    assert re.search(r"^all:.*lp_user", text, flags=re.M) and "lp_user.cc" in text
