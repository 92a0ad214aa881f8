"""CPU: the clumping / pruning surface without a GPU -- ABI, the float32 bound, rank construction, the sequential rule and
the .clumped / .prune.in / .prune.out writers."""
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_neighbor_and_select_symbols_declared_exported_and_bound():
    from ld_tools_amd import _lib
    header = (ROOT / "include" / "ldx.h").read_text()
    for name in ("ldx_ld_neighbors_workspace_bytes", "ldx_ld_neighbors_dev", "ldx_ld_select_workspace_bytes",
                 "ldx_ld_select_dev"):
        assert re.search(rf"\b{name}\s*\(", header), name
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.lib.ldx_version() == 102
    for n in (1, 129, 100_000):
        assert _lib.lib.ldx_ld_neighbors_workspace_bytes(n, 5008) == _lib.lib.ldx_ld_score_workspace_bytes(n, 5008)
        assert _lib.lib.ldx_ld_select_workspace_bytes(n) % 256 == 0 and _lib.lib.ldx_ld_select_workspace_bytes(n) >= 4 * n


def test_r2_bound_is_the_smallest_float32_that_passes():
    from ld_tools_amd.ops import r2_bound
    rng = np.random.default_rng(0)
    ts = np.concatenate([rng.uniform(1e-6, 1.0, 300), 10.0 ** -rng.uniform(0, 30, 100), [0.2, 0.5, 0.8, 1.0, 1e-45, 3.0]])
    for t in ts.tolist():
        for strict in (False, True):
            b = r2_bound(t, strict)
            assert b.dtype == np.float32 and float(b) > 0
            # every float32 s near the bound: s >= b exactly when s >= t (or s > t)
            s = (b.view(np.int32) + np.arange(-64, 65, dtype=np.int32)).view(np.float32)
            s = s[np.isfinite(s) & (s >= 0)]
            want = s.astype(np.float64) > t if strict else s.astype(np.float64) >= t
            assert np.array_equal(s >= b, want), (t, strict)
        # the float32 of t itself, and its nextafter neighbours, as thresholds
        f = np.float32(t)
        for g in (np.nextafter(f, np.float32(0)), f, np.nextafter(f, np.float32(1))):
            if float(g) > 0:
                assert r2_bound(float(g)) == g and r2_bound(float(g), True) == np.nextafter(g, np.float32(np.inf))


def test_r2_bound_rejects_non_positive_thresholds():
    from ld_tools_amd import LdxError
    from ld_tools_amd.ops import r2_bound
    for t in (0.0, -0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(LdxError):
            r2_bound(t)


def test_clump_ranks_ties_nan_and_degenerate():
    from ld_tools_amd import LdxError
    from ld_tools_amd.ops import NONE_U32, clump_ranks
    p = np.array([1e-5, 1e-8, np.nan, 1e-5, 0.02, 5e-3, 1e-8, 1e-9, 0.5])
    live = np.array([True, True, True, True, True, True, True, False, True])
    rank, ok = clump_ranks(p, 1e-4, 1e-2, live)
    # candidates by (p, row): rows 1, 6 (1e-8), 0, 3 (1e-5); row 7 is degenerate, row 2 NaN
    assert rank.dtype == np.uint32 and ok.dtype == np.uint8
    assert rank.tolist() == [2, 0, NONE_U32, 3, NONE_U32, NONE_U32, 1, NONE_U32, NONE_U32]
    assert ok.tolist() == [1, 1, 0, 1, 0, 1, 1, 0, 0]
    with pytest.raises(LdxError, match="p1 <= p2"):
        clump_ranks(p, 1e-2, 1e-4, live)
    with pytest.raises(LdxError, match="p1 <= p2"):
        clump_ranks(p, 0.0, 1e-4, live)
    with pytest.raises(LdxError, match="one p-value"):
        clump_ranks(p[:-1], 1e-4, 1e-2, live)
    with pytest.raises(LdxError, match="negative"):
        clump_ranks(-p, 1e-4, 1e-2, live)


def test_priority_ranks_descending_ties_by_row():
    from ld_tools_amd import LdxError
    from ld_tools_amd.ops import NONE_U32, priority_ranks
    pr = np.array([0.1, 0.3, 0.3, 0.0, 0.2, 0.3])
    live = np.array([True, True, False, True, True, True])
    assert priority_ranks(pr, live).tolist() == [3, 0, NONE_U32, 4, 2, 1]
    with pytest.raises(LdxError, match="NaN"):
        priority_ranks(np.array([0.1, np.nan]), np.array([True, True]))


def csr(adj, n):
    rows = [sorted(set(adj.get(i, []))) for i in range(n)]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return off, np.array([j for r in rows for j in r], dtype=np.int64)


def sym(edges):
    adj = {}
    for a, b in edges:
        adj.setdefault(a, []).append(b)
        adj.setdefault(b, []).append(a)
    return adj


def test_sequential_rule_on_hand_drawn_graphs():
    from ld_tools_amd.ops import NONE_U32, SEL_ASSIGNED, SEL_INDEX, SEL_OUT, select_host
    N = NONE_U32
    # a path 0-1-2-3-4, ranks along it: indices 0, 2, 4
    off, nbr = csr(sym([(0, 1), (1, 2), (2, 3), (3, 4)]), 5)
    st, own = select_host(off, nbr, np.array([0, 1, 2, 3, 4], np.uint32), np.ones(5, np.uint8))
    assert st.tolist() == [SEL_INDEX, SEL_ASSIGNED, SEL_INDEX, SEL_ASSIGNED, SEL_INDEX]
    assert own.tolist() == [0, 0, 2, 2, 4]
    # the same path ranked from the middle: 2 first takes 1 and 3; then 0 and 4
    st, own = select_host(off, nbr, np.array([1, 3, 0, 4, 2], np.uint32), np.ones(5, np.uint8))
    assert own.tolist() == [0, 2, 2, 2, 4] and st.tolist()[::2] == [SEL_INDEX] * 3
    # a star around 0 that is not a candidate; members need member_ok; a non-candidate goes to the first index of smaller rank
    off, nbr = csr(sym([(0, 1), (0, 2), (0, 3), (1, 4), (2, 4)]), 6)
    rank = np.array([N, 1, 0, 2, N, N], np.uint32)
    ok = np.array([1, 1, 1, 1, 0, 1], np.uint8)
    st, own = select_host(off, nbr, rank, ok)
    # 2 (rank 0) is an index and takes 0 (4 lacks member_ok); 1 and 3 are not neighbours of 2: both indices
    assert st.tolist() == [SEL_OUT, SEL_INDEX, SEL_INDEX, SEL_INDEX, SEL_OUT, SEL_OUT]
    assert own.tolist() == [2, 1, 2, 3, -1, -1]
    # a triangle with a pendant: 0-1-2-0, 2-3; ranks 3, 2, 1, 0 -> 3 first, takes 2; then 1 takes 0
    off, nbr = csr(sym([(0, 1), (1, 2), (2, 0), (2, 3)]), 4)
    st, own = select_host(off, nbr, np.array([3, 2, 1, 0], np.uint32), np.ones(4, np.uint8))
    assert own.tolist() == [1, 1, 3, 3] and st.tolist() == [SEL_ASSIGNED, SEL_INDEX, SEL_ASSIGNED, SEL_INDEX]


def test_clumped_writer_layout(tmp_path):
    from ld_tools_amd.drivers.clump import ClumpTable, write_clumped
    from ld_tools_amd.ops import Clumps
    owner = np.array([1, 1, -1, 1, 4, 1, 4, -1], dtype=np.int64)
    p = np.array([0.2, 1e-9, np.nan, 0.03, 5e-5, 0.004, 5e-5, 0.9])
    cl = Clumps(np.array([1, 4]), owner, np.array([2]), np.array([], dtype=np.int64), None, 1)
    tab = ClumpTable("6", [f"rs{k}" for k in range(8)], [100 * k + 5 for k in range(8)], p, cl)
    path = write_clumped(str(tmp_path / "x.clumped"), tab)
    text = Path(path).read_text()
    assert text == (" CHR    F          SNP         BP        P    TOTAL   NSIG    S05    S01   S001  S0001    SP2\n"
                    "   6    1          rs1        105    1e-09        3      1      1      1      0      0    rs0(1),rs3(1),rs5(1)\n"
                    "   6    1          rs4        405    5e-05        1      0      0      0      0      1    rs6(1)\n"
                    "\n\n")
    cl2 = Clumps(np.array([4]), np.array([-1, -1, -1, -1, 4, -1, -1, -1]), np.array([2]), np.array([], dtype=np.int64), None, 1)
    tab2 = ClumpTable("6", tab.rs_ids, tab.poss, p, cl2)
    lines = Path(write_clumped(str(tmp_path / "y.clumped"), tab2)).read_text().splitlines()
    assert lines[1].split() == ["6", "1", "rs4", "405", "5e-05", "0", "0", "0", "0", "0", "0", "NONE"]


def test_prune_writer_layout(tmp_path):
    from ld_tools_amd.drivers.prune import PruneTable, write_prune
    from ld_tools_amd.ops import Pruned
    keep = np.array([True, False, True, True, False])
    tab = PruneTable("1", ["rsA", "rsB", "rsC", "rsD", "rsE"], [1, 2, 3, 4, 5], Pruned(keep, None, None, 1))
    pin, pout = write_prune(str(tmp_path / "chr1"), tab)
    assert (pin, pout) == (str(tmp_path / "chr1.prune.in"), str(tmp_path / "chr1.prune.out"))
    assert Path(pin).read_text() == "rsA\nrsC\nrsD\n"
    assert Path(pout).read_text() == "rsB\nrsE\n"


def test_docstrings_say_what_the_files_are_not():
    import importlib
    clump = importlib.import_module("ld_tools_amd.drivers.clump")
    prune = importlib.import_module("ld_tools_amd.drivers.prune")
    assert "not PLINK's genotype-based estimate" in clump.__doc__
    assert "haplotype r" in prune.__doc__ and "not ``--indep-pairwise``'s sliding-window" in prune.__doc__
