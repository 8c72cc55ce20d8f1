"""CPU test: the row count above which coupling_bwd_r16_kernel's workgroups loop over tiles.

tests/test_gpu_nsc_tiles.py derives its batch sizes from that threshold (the launch's grid cap x the
rows of a backward workgroup).  A change to either must fail here, loudly, instead of silently turning
the tile-loop tests into single-pass runs.
"""
import re
from pathlib import Path

from tests.test_gpu_nsc_tiles import B_TILE_LOOP, BWD_GRID_CAP, BWD_ONE_PASS_ROWS, BWD_TILE_ROWS

CSRC = Path(__file__).resolve().parents[1] / "naz_amd" / "csrc"


def test_backward_tile_loop_threshold_is_what_the_gpu_tests_assume():
    train = (CSRC / "coupling_train.h").read_text()
    host = (CSRC / "coupling.hip").read_text()
    waves = re.findall(r"constexpr\s+int\s+kBwdWaves\s*=\s*(\d+)\s*;", train)
    assert len(waves) == 1, "kBwdWaves: definition not found in coupling_train.h"
    # the kernel's tile and the host's tile count are both 16 rows per wave
    assert re.search(r"ROWS\s*=\s*16\s*\*\s*kBwdWaves\b", train), "the backward tile is no longer 16 * kBwdWaves rows"
    m = re.search(r"static int bwd_layer\(.*?check_launch\(\"coupling_bwd_r16_kernel\"\)", host, re.S)
    assert m, "CouplingOps::bwd_layer not found in coupling.hip"
    body = m.group(0)
    assert re.search(r"ntiles\s*=\s*\(B \+ 16 \* kBwdWaves - 1\) / \(16 \* kBwdWaves\)", body), body
    cap = re.findall(r"grid\s*=\s*std::min<int64_t>\(ntiles,\s*(\d+)\)", body)
    assert len(cap) == 1, "the backward launch's grid cap not found"
    assert "dim3((unsigned)grid), dim3(kBwdWaves * 64)" in body
    assert int(cap[0]) == BWD_GRID_CAP and 16 * int(waves[0]) == BWD_TILE_ROWS
    assert BWD_ONE_PASS_ROWS == int(cap[0]) * 16 * int(waves[0]) == 131072
    # workgroups 0 and 1 take three tiles, the others two, and the last tile is partial
    ntiles = -(-B_TILE_LOOP // BWD_TILE_ROWS)
    assert ntiles == 2 * BWD_GRID_CAP + 2 and B_TILE_LOOP % BWD_TILE_ROWS == 37 and B_TILE_LOOP % 16 == 5
