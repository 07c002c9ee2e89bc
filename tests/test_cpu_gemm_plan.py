"""CPU-only: the GEMM launch planner (afx_gemm_plan, host arithmetic) under its two objectives.

Makespan (objective 0) is the dispatch every round up to now shipped: tests/golden/gemm_plan_makespan.txt holds what the commit
before the planner decided for every product of both models at B = 1, 7, 16, 64 and a grid around the dispatch thresholds
(tools/gemm_plan_table.py), and the planner must reproduce it line for line.  CU time (objective 1) must change the plan where
the tile arithmetic says it does, and the engine's chain launcher must follow the same objective."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from afx import _lib
    return _lib.lib()


def plan(lib, M, N, K, rpb=0, kchunk=0, groups=1, flags=0, objective=0):
    out = (C.c_int * 8)()
    assert lib.afx_gemm_plan(M, N, K, rpb, kchunk, groups, flags, objective, out) == 0
    return dict(zip(("family", "tile", "rows", "tiles", "split_rows", "rem_tile", "rem_tiles", "objective"), out))


def golden():
    rows = []
    for line in open(os.path.join(ROOT, "tests", "golden", "gemm_plan_makespan.txt")):
        if line.startswith("#") or not line.strip():
            continue
        v = [int(t) for t in line.split()]
        assert len(v) == 14
        rows.append((tuple(v[:7]), v[7:]))
    return rows


def test_makespan_plan_equals_the_parent_dispatch(lib):
    rows = golden()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gemm_plan_table
    finally:
        sys.path.pop(0)
    assert [r[0] for r in rows] == gemm_plan_table.shapes()  # the committed table covers the grid the tool names, in order
    shapes = {r[0][:3] for r in rows}
    for B in (1, 7, 16, 64):  # every trunk product of both models at B = 1, 7, 16, 64 is in it
        for N, K in ((3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096), (1024, 512)):
            assert (B * 199, N, K) in shapes
    bad = []
    for shape, want in rows:
        p = plan(lib, *shape, objective=0)
        got = [p[k] for k in ("family", "tile", "rows", "tiles", "split_rows", "rem_tile", "rem_tiles")]
        if got != want:
            bad.append((shape, want, got))
    assert not bad, bad[:10]
    assert len(rows) > 1000
    assert any(w[4] > 0 and w[5] == 0 for _, w in rows) and any(w[4] > 0 and w[5] == 82 for _, w in rows)  # both splits occur


@pytest.mark.parametrize("flags", [0, 2])
def test_cu_time_takes_full_height_tiles_for_the_student_batch(lib, flags):
    for N, K, t224, t256 in ((1024, 1024, 228, 200), (1024, 4096, 228, 200), (3072, 1024, 684, 600), (4096, 1024, 912, 800)):
        a, b = plan(lib, 12736, N, K, flags=flags, objective=0), plan(lib, 12736, N, K, flags=flags, objective=1)
        assert (a["tile"], a["rows"], a["tiles"], a["split_rows"]) == (77, 224, t224, 0)
        assert (b["tile"], b["rows"], b["tiles"], b["split_rows"]) == (7, 256, t256, 0)
        assert b["objective"] == 1 and a["objective"] == 0


def test_cu_time_conv_tile_and_ties(lib):
    # conv layer 6 of the student batch (fused LayerNorm epilogue): 199 tiles of 64 rows by makespan.  By CU time the model says
    # 100 of 128 rows, but that switch did not win its A/B (profiles/cu_time_dispatch_ab.txt) and is off in the default mask:
    # the shipped plan is the same under both objectives, and so are the two row splits
    a, b = plan(lib, 12736, 512, 1024, rpb=199, flags=1, objective=0), plan(lib, 12736, 512, 1024, rpb=199, flags=1, objective=1)
    assert (a["tile"], a["rows"], a["tiles"]) == (82, 64, 199) == (b["tile"], b["rows"], b["tiles"])
    for shape, want in golden():
        if want[4] > 0:
            b = plan(lib, *shape, objective=1)
            assert b["split_rows"] in (want[4], 0) and (b["split_rows"] == want[4] or b["tile"] == 7), (shape, want, b)
    # a small plain product (tests/test_gpu_cu_time_dispatch.py runs it): 16 x 16 tiles of 224 rows fill one round exactly, by CU
    # time 14 x 16 of 256 rows; 5 rows fewer leave both heights a ragged last tile.  (5 rows MORE need a 17th tile row of 224:
    # two rounds, so makespan takes 256 rows there as well.)
    for M in (3584, 3579):
        a, b = plan(lib, M, 4096, 128, objective=0), plan(lib, M, 4096, 128, objective=1)
        assert (a["rows"], a["tiles"]) == (224, 256) and (b["rows"], b["tiles"]) == (256, 224) and a["family"] == b["family"] == 7
    a, b = plan(lib, 3589, 4096, 128, objective=0), plan(lib, 3589, 4096, 128, objective=1)
    assert (a["rows"], a["tiles"]) == (256, 240) == (b["rows"], b["tiles"])
    # a tie goes to the taller tile: 2900 rows are 12 tiles of 256 rows x 13 units = 156 per column block and 13 tiles of 224
    # rows x 12 = 156 as well (16 of 192 x 11 = 176, 19 of 160 x 10 = 190)
    assert plan(lib, 2900, 4096, 1024, objective=1)["rows"] == 256
    # under CU time no product of the table takes more tile slots x unit than under makespan
    unit = {7: 13, 77: 12, 76: 11, 75: 10, 8: 10, 83: 9, 82: 8}
    for shape, _ in golden():
        a, b = plan(lib, *shape, objective=0), plan(lib, *shape, objective=1)
        if a["tile"] in unit and b["tile"] in unit and not a["split_rows"] and not b["split_rows"]:
            assert b["tiles"] * unit[b["tile"]] <= a["tiles"] * unit[a["tile"]], (shape, a, b)


def test_chain_waves_follow_the_objective(lib):
    assert lib.afx_conf_chain_waves(12800, 0) == 4 and lib.afx_conf_chain_waves(12800, 1) == 8  # B = 64: 200 -> 100 workgroups
    assert lib.afx_conf_chain_waves(153, 0) == 4 and lib.afx_conf_chain_waves(153, 1) == 8       # 3 -> 2
    assert lib.afx_conf_chain_waves(64, 1) == 4 and lib.afx_conf_chain_waves(16, 1) == 4         # one workgroup either way
    assert lib.afx_conf_chain_waves(40000, 1) == 8 and lib.afx_conf_chain_waves(40000, 0) == 4  # 313 x 30.9 against 625 x 27.3
