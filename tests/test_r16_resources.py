"""CPU test: the config-3 log_prob instance of coupling_r16_kernel keeps its register budget.

Its GEMM stages prefetch their A fragments with untracked LDS reads (gemm_r16_pf); that only pays
while the kernel holds four waves per SIMD with nothing in scratch, so the code object's kernel
metadata must say: no private segment, at most 128 VGPRs.
"""
import re
import subprocess
import tempfile
from pathlib import Path

import pytest

from tests.isa_ring import LLVM, code_objects

LIB = Path(__file__).resolve().parents[1] / "naz_amd" / "lib" / "libnazhip.so"
HEADLINE = "_ZN3naz19coupling_r16_kernelINS_6CfgR16ILi16ELi32ELi8ELi8ELi128ELb1EEELb1ELi0EE"


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        from naz_amd import build
        build.build()
    return LIB


def kernel_metadata(co: bytes) -> dict:
    """kernel symbol -> {key: value} of the scalar entries of its amdhsa.kernels record."""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(co)
        f.flush()
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", f.name], check=True, capture_output=True,
                               text=True).stdout
    out, cur = {}, None
    for line in notes.splitlines():
        m = re.match(r"^  - \.(\w+):\s*(.*)$", line)  # first key of a kernel record
        if m:
            cur = {m.group(1): m.group(2).strip()}
            continue
        m = re.match(r"^    \.(\w+):\s*(.*)$", line)  # further scalar keys of the record
        if m and cur is not None:
            cur[m.group(1)] = m.group(2).strip()
            if m.group(1) == "name":
                out[m.group(2).strip()] = cur
    return out


def test_headline_kernel_has_no_scratch_and_fits_128_vgprs(lib):
    found = []
    for co in code_objects(lib):
        for name, md in kernel_metadata(co).items():
            if name.startswith(HEADLINE):
                found.append((name, md))
    assert len(found) == 1, f"config-3 log_prob kernel: {len(found)} records found"
    md = found[0][1]
    assert int(md["private_segment_fixed_size"]) == 0, md
    assert int(md["vgpr_count"]) <= 128, md
