"""The kernel library is built from three translation units (csrc/Makefile UNITS).  That only stays sound while every header
says what it needs - each ``csrc/*.h`` compiles on its own - and while no kernel header is compiled into two units."""
import glob
import os
import subprocess

import pytest

from catre_amd import hip, resusage

CSRC = os.path.dirname(hip.LIB_PATH)
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.h")))


def _make_var(target):
    return subprocess.run(["make", "-s", "--no-print-directory", "-C", CSRC, target], check=True, capture_output=True,
                          text=True).stdout.split()


def test_every_header_is_listed():
    assert len(HEADERS) >= 28 and "catre_device.h" in HEADERS and "catre_host.h" in HEADERS, HEADERS


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone(header, tmp_path):
    """A one-line file that includes only this header, with the Makefile's compiler, architecture and flags."""
    src = tmp_path / "alone.hip"
    src.write_text(f'#include "{os.path.join(CSRC, header)}"\n')
    hipcc, arch = _make_var("print-hipcc"), _make_var("print-arch")
    out = subprocess.run(hipcc + [f"--offload-arch={arch[0]}"] + _make_var("print-flags") + ["-fsyntax-only", str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]


def test_no_kernel_is_defined_twice_and_the_resource_table_lists_every_kernel():
    if not os.path.exists(resusage.RAW) or not os.path.exists(hip.LIB_PATH) or \
            os.path.getmtime(resusage.RAW) + 120 < os.path.getmtime(hip.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    if not os.path.exists(resusage.OBJDUMP):
        pytest.skip("llvm-objdump not in this image")
    isa = resusage.disassemble(hip.LIB_PATH)  # raises on a symbol that two code objects define
    rows = [r["mangled"] for r in resusage.parse()]
    assert len(rows) == len(set(rows)), sorted(r for r in set(rows) if rows.count(r) > 1)[:5]
    assert set(isa) == set(rows), (sorted(set(isa) - set(rows))[:5], sorted(set(rows) - set(isa))[:5])
