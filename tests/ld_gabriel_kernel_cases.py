"""Inputs and a direct harness for the integer kernels of csrc/ldx_gabriel.hip (tests/test_ld_gabriel_host.py,
tests/test_gpu_ld_gabriel.py) -- TEST INFRASTRUCTURE ONLY, a plain module like tests/ld_gabriel_cases.py.  No panel and no EM:
the bound bytes are made up, so the shapes that a panel never reaches can be built at will.

  * random_bounds / chain_bounds / CASES: seeded bound bands in the layout of ops.band_layout_host.  Every case is a read-only
    dict, built once per process (case(name)); the host mirrors on it are cached the same way (mirrors(name, ...)).
  * column_major: the (first, last) of every slot of the candidate list, from the layout alone.
  * settle_profile / late_rejections: plain-Python restatements of the pick rule, chunk by chunk of 256.  They PROVE that an
    input reaches a depth (rounds inside a chunk, a block of an earlier chunk killing a candidate); they are no expected value.
  * Kernels: ldx_gabriel_candidates_dev, the caller's stable sort, ldx_gabriel_pick_dev, on views carved from ONE uint8
    allocation filled with a poison byte; every view is followed by a gap of at least 256 bytes that must still hold it.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

CHUNK = 256                       # candidates per trip of pick_kernel, SNPs per trip of scan_kernel and of the numbering
POISON = 0xA5
GAP = 256
STEPS = (0, 300, 700, 2500)
KINDS = (0.55, 0.15, 0.2, 0.1)    # strong, recombinant, uninformative, no interval
OTHER = dict(cuts=(75, 60, 55, 65), max_spans=(1500, 4000, 6000, None), min_informative=(1, 2, 4, 5), strong_share=(3, 4),
             cand_cut=60, strong_hi=97, recomb_hi=85)          # the non-default set of the host test
SCALE = 1 << 33                   # the 64-bit case: positions, window and span caps times 2^33
SCALED = dict(max_spans=(20_000 * SCALE, 30_000 * SCALE, None, None))


def _frozen(**kw):
    for v in kw.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return kw


def _case(pos, window, kept, lo, hi):
    from ld_tools_amd import ops
    band_lo, off = ops.band_layout_host(pos, window)
    assert lo.shape == hi.shape == (int(off[-1]),)
    return _frozen(pos=pos, window=int(window), kept=kept, lo=lo, hi=hi, band_lo=band_lo, off=off, n=int(pos.shape[0]),
                   n_cells=int(off[-1]))


def random_bounds(n: int, window: int, seed: int, kinds=KINDS, steps=STEPS, step_p=None, drop: float = 0.15):
    """Random bytes for the bounds: a pair is strong (lo 45 .. 99, hi 96 .. 100), recombinant (hi below 90), uninformative or
    without an interval with the probabilities ``kinds``; position steps drawn from ``steps`` (a step of 0: two SNPs at one
    position); about ``drop`` of the SNPs not kept."""
    from ld_tools_amd import ops
    rng = np.random.default_rng(seed)
    pos = np.cumsum(rng.choice(steps, size=n, p=step_p)).astype(np.int64)
    kept = rng.random(n) > drop
    m = int(ops.band_layout_host(pos, window)[1][-1])
    kind = rng.choice(4, size=m, p=kinds)
    lo = np.select([kind == 0, kind == 1, kind == 2], [rng.integers(45, 100, m), rng.integers(0, 40, m), rng.integers(0, 70, m)],
                   ops.NO_CI).astype(np.uint8)
    hi = np.select([kind == 0, kind == 1, kind == 2], [rng.integers(96, 101, m), rng.integers(40, 90, m), rng.integers(90, 101, m)],
                   ops.NO_CI).astype(np.uint8)
    return _case(pos, window, kept, lo, hi)


def chain_bounds(n: int, window: int, kept=None, strong=None):
    """Positions 0 .. n - 1 and the bounds (99, 100) in every cell -- strong at every cut --, or only in the cells ``strong``
    (bool [n_cells]) with no interval elsewhere.  In SNP units nearly every span ties: the order of the pick is the slot
    order and the caller's stable sort, nothing else."""
    from ld_tools_amd import ops
    pos = np.arange(n, dtype=np.int64)
    m = int(ops.band_layout_host(pos, window)[1][-1])
    strong = np.ones(m, dtype=bool) if strong is None else np.asarray(strong, dtype=bool)
    kept = np.ones(n, dtype=bool) if kept is None else np.asarray(kept, dtype=bool)
    return _case(pos, window, kept, np.where(strong, 99, ops.NO_CI).astype(np.uint8), np.where(strong, 100, ops.NO_CI).astype(np.uint8))


def random_keep(n: int, seed: int, drop: float = 0.15) -> np.ndarray:
    return np.random.default_rng(seed).random(n) > drop


def _some_cells(m: int, count: int, seed: int) -> np.ndarray:
    strong = np.zeros(m, dtype=bool)
    strong[np.random.default_rng(seed).choice(m, size=count, replace=False)] = True
    return strong


def _scaled(name: str):
    c = case(name)
    return _case(c["pos"] * SCALE, c["window"] * SCALE, c["kept"], c["lo"], c["hi"])


TRIP_SIZES = (1, 2, 255, 256, 257, 512, 513)
CHAINS = ((600, 1), (600, 2), (1500, 3), (20_000, 1), (601, 1))
MOSTLY_STRONG = (0.93, 0.01, 0.03, 0.03)
CASES = {
    # 1. with the brute reference: a 21 kb step now and then, so that the 20 kb cap of a two-SNP block bites inside the window
    "random257": lambda: random_bounds(257, 25_000, 7,kinds=(0.8, 0.04, 0.1, 0.06), steps=STEPS + (21_000,),
                                       step_p=(0.24, 0.24, 0.24, 0.24, 0.04)),
    "random513": lambda: random_bounds(513, 9_000, 12, kinds=(0.8, 0.04, 0.1, 0.06)),
    # 2. many chunks of candidates
    "long3000": lambda: random_bounds(3000, 9_000, 21, kinds=MOSTLY_STRONG),
    "wide600": lambda: random_bounds(600, 60_000, 22, kinds=(0.9, 0.01, 0.05, 0.04)),
    # 6. every span above 2^32
    "scaled513": lambda: _scaled("random513"),
    # 8. no pair in any window
    "empty700": lambda: _case(3 * np.arange(700, dtype=np.int64) + 5, 0, random_keep(700, 8), np.zeros(0, dtype=np.uint8),
                              np.zeros(0, dtype=np.uint8)),
    # 4. valid candidates at the chunk boundary: exactly 256 and exactly 512 with dead slots behind them, and lists without a
    # single dead slot whose length is a multiple of 256
    "valid256of512": lambda: chain_bounds(513, 1, strong=_some_cells(512, 256, 41)),
    "valid512of699": lambda: chain_bounds(700, 1, strong=_some_cells(699, 512, 42)),
    "full256": lambda: chain_bounds(257, 1),
    "full512": lambda: chain_bounds(513, 1),
}
CASES.update({f"chain{n}w{w}": (lambda n=n, w=w: chain_bounds(n, w)) for n, w in CHAINS})                       # 3.
CASES.update({f"trip{n}": (lambda n=n: chain_bounds(n, 1, kept=random_keep(n, 100 + n))) for n in TRIP_SIZES})  # 4.
_BUILT, _MIRRORS = {}, {}


def case(name: str) -> dict:
    if name not in _BUILT:
        _BUILT[name] = CASES[name]()
    return _BUILT[name]


def mirrors(name: str, params=None, all_kept: bool = False):
    """(cands int64 [k, 3], block_of uint32 [n], n_blocks): ops.gabriel_candidates_host and ops.gabriel_pick_host on a case,
    with ``params`` (None: the defaults) and the case's kept mask (``all_kept``: every SNP).  Read-only, computed once."""
    from ld_tools_amd import ops
    key = (name, None if not params else tuple(sorted(params.items())), all_kept)
    if key not in _MIRRORS:
        c = case(name)
        kept = np.ones(c["n"], dtype=bool) if all_kept else c["kept"]
        cands = ops.gabriel_candidates_host(c["lo"], c["hi"], c["pos"], kept, c["window"], **(params or {}))
        block_of, n_blocks = ops.gabriel_pick_host(cands, c["n"], kept)
        cands.setflags(write=False)
        block_of.setflags(write=False)
        _MIRRORS[key] = (cands, block_of, n_blocks)
    return _MIRRORS[key]


def brute(name: str, params=None, all_kept: bool = False):
    """(valid, lost, block_of, accepted, overlapped): ld_gabriel_cases.brute_candidates and brute_pick on a case -- plain loops
    over every pair, no suffix counts.  Computed once."""
    import ld_gabriel_cases as gc
    key = ("brute", name, None if not params else tuple(sorted(params.items())), all_kept)
    if key not in _MIRRORS:
        c = case(name)
        kept = np.ones(c["n"], dtype=bool) if all_kept else c["kept"]
        lo_d = gc.dense_from_band(c["lo"], c["band_lo"], c["off"], c["n"])
        hi_d = gc.dense_from_band(c["hi"], c["band_lo"], c["off"], c["n"])
        valid, lost = gc.brute_candidates(lo_d, hi_d, c["pos"], kept, c["window"], **(params or {}))
        block_of, accepted, overlapped = gc.brute_pick(valid, c["n"], kept)
        block_of.setflags(write=False)
        _MIRRORS[key] = (valid, lost, block_of, accepted, overlapped)
    return _MIRRORS[key]


def column_major(band_lo, offsets):
    """(first, last, cell), each [n_cells]: the pair of every slot of the candidate list -- the cells of the layout ordered by
    column (first), then row (last) -- and the cell of the band that the slot reads."""
    off = np.asarray(offsets).astype(np.int64)
    blo = np.asarray(band_lo).astype(np.int64)
    rows = np.repeat(np.arange(blo.shape[0]), np.diff(off))
    cols = np.arange(off[-1]) - off[rows] + blo[rows]
    order = np.lexsort((rows, cols))
    return cols[order], rows[order], order


def pick_order(cands) -> np.ndarray:
    """The valid candidates in the order the pick visits them: span descending, then smaller first, then smaller last."""
    cands = np.asarray(cands, dtype=np.int64).reshape(-1, 3)
    return cands[np.lexsort((cands[:, 1], cands[:, 0], -cands[:, 2]))]


def settle_profile(cands, n: int):
    """(chunks, the most rounds any chunk needs) of the pick over ``cands`` (rows first, last, span IN PICK ORDER), 256 at a time.
    A candidate that touches a block of an earlier chunk is dead on entry.  Then rounds: everybody looks at the states the
    EARLIER candidates of the chunk had after the round before -- dead with an accepted one that overlaps it, accepted once no
    overlapping one is undecided, waiting otherwise -- until nobody waits.  A chunk runs at least one round."""
    DEAD, OPEN, TAKEN = 0, 1, 2
    used = [False] * n
    chunks, deepest = 0, 0
    cands = [(int(f), int(l)) for f, l, _ in cands]
    for base in range(0, len(cands), CHUNK):
        chunk = cands[base:base + CHUNK]
        chunks += 1
        state = [DEAD if any(used[f:l + 1]) else OPEN for f, l in chunk]
        earlier = [[t for t in range(k) if not (chunk[k][0] > chunk[t][1] or chunk[t][0] > chunk[k][1])] for k in range(len(chunk))]
        rounds = 0
        while True:
            rounds += 1
            new = list(state)
            for k in range(len(chunk)):
                if state[k] != OPEN:
                    continue
                seen = [state[t] for t in earlier[k]]
                new[k] = DEAD if TAKEN in seen else OPEN if OPEN in seen else TAKEN
            state = new
            if OPEN not in state:
                break
        deepest = max(deepest, rounds)
        for (f, l), st in zip(chunk, state):
            if st == TAKEN:
                used[f:l + 1] = [True] * (l + 1 - f)
    return chunks, deepest


def late_rejections(cands, n: int):
    """[(rank, first, last, chunk of the block in its way)] of the candidates (rows IN PICK ORDER) that the greedy rule rejects
    because of a block accepted in an EARLIER chunk of 256 -- what only the `used` bytes carry from chunk to chunk."""
    owner = [None] * n
    out = []
    for rank, (f, l, _) in enumerate(np.asarray(cands).tolist()):
        hit = [owner[s] for s in range(f, l + 1) if owner[s] is not None]
        if not hit:
            owner[f:l + 1] = [rank // CHUNK] * (l + 1 - f)
        elif min(hit) < rank // CHUNK:
            out.append((rank, f, l, min(hit)))
    return out


def nested_list(n: int = 600, seed: int = 5):
    """(span, first, last, block_of, n_out): a list for the pick alone, on n - 1 slots.  The pairs (2 k + 2, 2 k + 3), k < 256,
    span 9, fill the first chunk; the second opens with (1, 514), span 5, whose two ends are free and whose inside is all
    blocks, then (0, 1), span 4, and (514, 515), span 3, which are accepted only if (1, 514) is not.  No list of the candidates
    kernel looks like this -- a block never lies strictly inside a later candidate when spans are distances of sorted
    positions -- but the pick promises "no SNP in [first, last] lies in an accepted block" for the spans it is given.  The
    live slots are scattered among dead ones in this order; the expected result is written out by hand."""
    from ld_tools_amd import ops
    live = [(2 * k + 2, 2 * k + 3, 9) for k in range(CHUNK)] + [(1, 514, 5), (0, 1, 4), (514, 515, 3)]
    slots = np.sort(np.random.default_rng(seed).choice(n - 1, size=len(live), replace=False))
    span = np.full(n - 1, -1, dtype=np.int64)
    first = np.zeros(n - 1, dtype=np.uint32)
    last = np.ones(n - 1, dtype=np.uint32)
    first[slots], last[slots], span[slots] = np.array(live).T
    block_of = np.full(n, ops.NO_BLOCK, dtype=np.uint32)
    block_of[0:2] = 0
    block_of[2:514] = 1 + np.arange(512) // 2
    block_of[514:516] = 257
    return span, first, last, block_of, [258, len(live)]


# ---- the kernels, directly -------------------------------------------------------------------------------------------------------
Result = namedtuple("Result", "cand_span cand_first cand_last block_of n_out")


def _up(v: int) -> int:
    return (v + 255) // 256 * 256


class Kernels:
    """One carve for one case.  Views, each followed by a gap: the two bound bands, positions, keep, the layout, the three
    candidate arrays, the two workspaces at exactly their *_workspace_bytes, block_of, n_out.  ``layout`` = (band_lo, offsets)
    replaces the case's own (a foreign layout: the bands, the list and n_cells stay the case's)."""

    def __init__(self, device, c: dict, keep="case", layout=None, fill: int = POISON):
        import torch
        from ld_tools_amd import _lib
        self.torch, self.lib, self.check = torch, _lib.lib, _lib.check
        self.c, self.n, self.n_cells = c, c["n"], c["n_cells"]
        self.keep = c["kept"] if isinstance(keep, str) else keep            # None: the calls get a null pointer
        self.layout = (c["band_lo"], c["off"]) if layout is None else layout
        n, m = self.n, self.n_cells
        self.cand_ws = int(self.lib.ldx_gabriel_candidates_workspace_bytes(n, m))
        self.pick_ws = int(self.lib.ldx_gabriel_pick_workspace_bytes(n))
        assert self.cand_ws % 256 == 0 and self.pick_ws % 256 == 0
        sizes = [("ci_lo", m), ("ci_hi", m), ("pos", 8 * n), ("keep", n if self.keep is not None else 0), ("band_lo", 4 * n),
                 ("offsets", 8 * (n + 1)), ("cand_span", 8 * m), ("cand_first", 4 * m), ("cand_last", 4 * m),
                 ("cand_ws", self.cand_ws), ("pick_ws", self.pick_ws), ("block_of", 4 * n), ("n_out", 8)]
        self.at, end = {}, GAP                                               # (a gap in front of the first view, too)
        for name, size in sizes:
            self.at[name] = (end, size)
            end = _up(end + size) + GAP
        self.whole = torch.empty(end + 256, dtype=torch.uint8, device=device)
        shift = -self.whole.data_ptr() % 256                                # (the workspaces must be 256-byte aligned)
        self.buf = self.whole[shift:shift + end]
        assert self.buf.data_ptr() % 256 == 0
        self.is_gap = np.ones(end, dtype=bool)
        for a, size in self.at.values():
            self.is_gap[a:a + size] = False
        self.refill(fill)

    def refill(self, fill: int) -> None:
        """``fill`` into every byte -- outputs, workspaces and gaps --, then the inputs."""
        self.fill = fill
        self.buf.fill_(fill)
        c = self.c
        inputs = dict(ci_lo=c["lo"], ci_hi=c["hi"], pos=c["pos"].astype(np.int64), band_lo=np.asarray(self.layout[0]).astype(np.uint32),
                      offsets=np.asarray(self.layout[1]).astype(np.uint64))
        if self.keep is not None:
            inputs["keep"] = np.asarray(self.keep).astype(np.uint8)
        for name, values in inputs.items():
            self._put(name, values)

    def view(self, name: str, dtype=None):
        a, size = self.at[name]
        v = self.buf[a:a + size]
        return v if dtype is None else v.view(dtype)

    def ptr(self, name: str):
        a, size = self.at[name]
        return self.buf.data_ptr() + a if size else None

    def _put(self, name: str, values) -> None:
        a, size = self.at[name]
        raw = np.ascontiguousarray(values).view(np.uint8).reshape(-1)
        assert raw.shape[0] == size, name
        if size:
            self.buf[a:a + size].copy_(self.torch.from_numpy(raw.copy()))

    def _pick(self, keep: bool) -> None:
        m = self.n_cells
        if m:                                                               # the caller's part of the contract (include/ldx.h)
            sorted_span, order = self.torch.sort(self.view("cand_span", self.torch.int64), descending=True, stable=True)
        self.check(self.lib.ldx_gabriel_pick_dev(
            sorted_span.data_ptr() if m else None, order.data_ptr() if m else None, self.ptr("cand_first"), self.ptr("cand_last"),
            m, self.ptr("keep") if keep else None, self.n, self.ptr("block_of"), self.ptr("n_out"), self.ptr("pick_ws"),
            self.pick_ws, None), "ldx_gabriel_pick_dev")

    def _collect(self, pick: bool) -> Result:
        self.torch.cuda.synchronize()
        host = self.buf.cpu().numpy()
        stray = np.flatnonzero(self.is_gap & (host != self.fill))
        assert stray.size == 0, f"{stray.size} bytes of the gaps were written, the first at {stray[0]} of {self.at}"

        def get(name, dtype):
            a, size = self.at[name]
            return host[a:a + size].copy().view(dtype)

        return Result(get("cand_span", np.int64), get("cand_first", np.uint32), get("cand_last", np.uint32),
                      get("block_of", np.uint32) if pick else None, get("n_out", np.uint32) if pick else None)

    def run(self, params=None, cand_keep: bool = True, pick_keep: bool = True, pick: bool = True) -> Result:
        """The candidates call, the caller's stable sort, the pick call (``pick`` False: the candidates call alone); then every
        gap must hold the fill.  ``params``: a dict for ops.gabriel_params, None for a null pointer.  ``cand_keep`` /
        ``pick_keep`` False: that call gets a null keep whatever the carve holds."""
        from ld_tools_amd import ops
        prm = None if params is None else ops._gabriel_struct(ops.gabriel_params(**params))
        self.check(self.lib.ldx_gabriel_candidates_dev(
            self.ptr("ci_lo"), self.ptr("ci_hi"), self.ptr("band_lo"), self.ptr("offsets"), self.n_cells, self.ptr("pos"),
            self.ptr("keep") if cand_keep else None, self.n, self.c["window"], None if prm is None else C.addressof(prm),
            self.ptr("cand_span"), self.ptr("cand_first"), self.ptr("cand_last"), self.ptr("cand_ws"), self.cand_ws, None),
            "ldx_gabriel_candidates_dev")
        if pick:
            self._pick(pick_keep)
        return self._collect(pick)

    def pick_list(self, span, first, last, keep: bool = True) -> Result:
        """The sort and the pick call alone on a list of the caller's: one (span, first, last) per slot of the carve, -1 for
        a dead slot.  The pick takes the spans as given; they need not be distances of the case's positions."""
        self._put("cand_span", np.asarray(span, dtype=np.int64))
        self._put("cand_first", np.asarray(first, dtype=np.uint32))
        self._put("cand_last", np.asarray(last, dtype=np.uint32))
        self._pick(keep)
        return self._collect(True)
