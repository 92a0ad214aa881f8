"""Batched LD operators over a PackedPanel -- the host-side mirror of the reference's pair loops.

    ld_triangle(panel)                      <- ld_triangle.py:133-230  (all row > col pairs)
    ld_area(panel, positions, queries, ...) <- ld_area.py:152-276      (windowed scan, thresholded hits)
    ld_score(panel, positions, ...)         LD scores: windowed sums of r^2 per SNP (LDSC's l2), optionally per category
    ld_matvec(panel, x, positions, ...)     R x (or R^2 x) over the window for up to 8 vectors, without the matrix
    ld_ridge(panel, z, positions, ...)      (R + lam I) beta = z by conjugate gradients on ld_matvec
    ld_band(panel, positions, ...)          the windowed LD matrix KEPT: signed r of every in-window pair, 4 bytes each
    ld_cross_score(band_a, band_b)          cross-panel LD scores (sum of r1 r2 over the window) from two stored bands
    ld_cross / ld_regions                   the cross-LD profile of the band and the LD-independent regions cut from it
    ld_neighbors(panel, positions, ...)     per-SNP lists of the SNPs in the window with r^2 above a threshold
    ld_clump / ld_prune                     greedy clumping (PLINK --clump) and priority pruning on those lists
    ld_rect(panel_i, panel_j)               signed r of every SNP of one set against every SNP of another (dense float32)
    ld_rect_hits(panel_i, panel_j, r2=...)  the pairs of that rectangle with r^2 above a threshold, as a CSR
    ld_em(panel_i, panel_j)                 unphased LD by maximum likelihood: EM r and D' of two SNP sets (dense float32)
    ld_em_hits(panel_i, panel_j, r2=...)    the pairs of that rectangle whose EM r^2 reaches a threshold, with their D'
                                            (both: missing="pairwise" = over the individuals called at both SNPs)
    ld_em_band(panel, positions, ...)       the EM r and D' of every in-window pair of ONE panel, kept in ld_band's layout;
                                            ld_neighbors / ld_clump / ld_prune(em=True) are the lists and selections on them
    ld_decay / ld_blocks                    LD decay curves per distance bin; haplotype blocks by the four-gamete test
    ld_dprime_ci / ld_gabriel_blocks        D' confidence bounds on the EM band and Gabriel's haplotype blocks
    sample_counts / king_kinship / ibs_matrix   IBS counts and KING-robust kinship between the individuals
    sample_wprod / ld_grm / grm_cutoff      weighted genotype x genotype sums on the int8 matrix cores; the genetic relationship matrix
    GenoOperator / geno_matmul / geno_rmatmul   genotype products on the matrix cores, exact integers
    sample_pca / polygenic_score            sample PCA and per-SNP weights applied to the individuals, on those products
    ld_glm(panel, Y, covar, ...)            linear association scan on the reverse genotype product
    ld_glm_logistic(panel, Y, covar, ...)   logistic association scan for 0/1 traits: a Newton fit per cell on the fp64 matrix cores;
                                            firth="fallback" / "always": Firth's penalised fit where that has no finite maximiser / everywhere
    geno_group_counts(panel, groups)        genotype counts of every SNP within each of up to 32 groups of individuals, one pass
    ld_hardy / ld_model / ld_test_missing   exact HWE test per group; the table tests of --model and Fisher's test; missingness by status
    sample_qc / snp_qc_mask / sample_qc_mask   per-individual call counts and F; the --maf / --geno / --hwe and --mind masks
    ld_mperm(panel, case, n_perm=, seed=)   max(T) permutation test of the allelic / trend test: EMP1 and EMP2, the SNP x permutation
                                            rectangle reduced on chip to n counters and R maxima
    pair_counts(panel_i, panel_j)           <- calc_ld.py:32           (bit-exact n11 block)
    ld_from_counts(n, n11, a1, r1, a2, r2)  <- calc_ld.py:33-97        (the epilogue alone)

Every device function enqueues HIP kernels of libldx.so on torch's current stream and returns device tensors.  The
``*_host`` functions are the numpy mirrors the tests compare against; each stands next to the call it mirrors.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import MEASURES, UNIT_PAIRS, check, lib
from .panel import PackedPanel, _ptr, _stream_ptr, require_gpu, select_index


PATHS = {"auto": 0, "popcount": 1, "mfma": 2, "fp4": 3}


def set_triangle_path(name: str) -> None:
    """Choose the kernel behind ld_triangle: 'popcount', 'mfma' or 'auto' (results are identical)."""
    check(lib.ldx_set_triangle_path(PATHS[name]), "ldx_set_triangle_path")


def get_triangle_path() -> str:
    code = lib.ldx_get_triangle_path()
    return next(k for k, v in PATHS.items() if v == code)


def set_area_path(name: str) -> None:
    """Choose the kernel behind ld_area: 'popcount' (scan of the query rows), 'mfma' (the whole +-flank band on the
    matrix pipe) or 'auto' (mfma when at least 1/16 of the SNPs are queries).  The hit sets are identical."""
    check(lib.ldx_set_area_path(PATHS[name]), "ldx_set_area_path")


def get_area_path() -> str:
    code = lib.ldx_get_area_path()
    return next(k for k, v in PATHS.items() if v == code)


def _band_path(path: Optional[str]) -> int:
    """The band operators' path code: the FP4 band unless another is named."""
    return PATHS["fp4" if path is None else path]


def _ws(workspace: torch.Tensor) -> Tuple[int, int]:
    """A workspace's two arguments of a library entry: its address and its size in bytes."""
    return workspace.data_ptr(), workspace.numel() * workspace.element_size()


def _band_workspace(size_fn, panel: PackedPanel, workspace: Optional[torch.Tensor]) -> torch.Tensor:
    """A band operator's workspace: the caller's, checked against ``size_fn`` (its ldx_ld_*_workspace_bytes), or a new one
    (the call's first kernels set what they read: no initialisation)."""
    need = size_fn(panel.n_snps, panel.n_hap)
    if workspace is None:
        return torch.empty(need, dtype=torch.uint8, device=panel.device)
    if _ws(workspace)[1] < need:
        raise _lib.LdxError(f"workspace too small: {need} bytes needed")
    return workspace


def _phased_panel(panel: PackedPanel) -> tuple:
    """The panel's arguments of the phased band entries: alt, acnt, rcnt, fa, fr."""
    return (panel.alt.data_ptr(), panel.acnt.data_ptr(), panel.rcnt.data_ptr(), panel.fa.data_ptr(),
            panel.fr.data_ptr())


def _dosage_panel(panel: PackedPanel) -> tuple:
    """The panel's arguments of the genotype-dosage entries: alt, gstat (PackedPanel.dosage_stats, cached on the panel)."""
    return panel.alt.data_ptr(), panel.dosage_stats()[1].data_ptr()


def _keep_mask(keep, n: int) -> Optional[np.ndarray]:
    if keep is None:
        return None
    k = keep.cpu().numpy() if isinstance(keep, torch.Tensor) else np.asarray(keep)
    if k.shape != (n,) or (k.dtype != bool and not np.isin(k, (0, 1)).all()):
        raise _lib.LdxError(f"keep must be a boolean array of shape [{n}]")
    return k.astype(bool)


def _keep_dev(keep, n: int, dev) -> Optional[torch.Tensor]:
    """_keep_mask as the entries take it: a contiguous uint8 tensor [n] on ``dev``, None for no mask."""
    k = _keep_mask(keep, n)
    return None if k is None else torch.from_numpy(k.astype(np.uint8)).to(dev)


def _even_n_hap(what: str, panel: PackedPanel) -> None:
    """The operators over individuals need both haplotypes of each one."""
    if panel.n_hap % 2:
        raise _lib.LdxError(f"{what}: n_hap must be even (haplotypes 2a and 2a + 1 are individual a), got {panel.n_hap}")


def _plan_workspace(size_fn, panel: PackedPanel, workspace: Optional[torch.Tensor]) -> torch.Tensor:
    """_band_workspace for the plan bands (pairwise-complete and EM), whose ``size_fn`` takes the SNP count alone."""
    return _band_workspace(lambda n, _h: size_fn(n), panel, workspace)


def _band_layout(pos: torch.Tensor, n: int, window: int, dev) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """A stored band's layout on the device (ldx_ld_band_layout_dev): ``(lo int32 [n], offsets int64 [n + 1], n_cells)``; the
    total, offsets[n], is read back -- the one synchronisation of the band calls."""
    lo = torch.empty(n, dtype=torch.int32, device=dev)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    check(lib.ldx_ld_band_layout_dev(pos.data_ptr(), n, window, lo.data_ptr(), offsets.data_ptr(), _stream_ptr()),
          "ldx_ld_band_layout_dev")
    return lo, offsets, int(offsets[n].item())


# --------------------------------------------------------------------------- triangle
@dataclass
class TriangleResult:
    """Strip-packed lower triangle of one panel (layout: include/ldx.h, "Triangle work units").

    The cells are in ONE of the formats of include/ldx.h: ``ld32`` (float32 nearest to k / 10^4, -0.0 = the
    reference's int 0, 8 bytes per pair), ``k16`` (k itself in 15 bits + an int-0 bit, 4 bytes per pair) or -- one measure
    only, 2 bytes per pair, what a table writer needs (ld_triangle.py:223-230,344-360 print ONE measure) -- ``k16r`` /
    ``k16d`` (the r_square / d_prime half of k16).  Values a format cannot hold (>= 1024 / >= 3.2767: only with missing
    codes) are escape cells; ``dense_values()`` resolves them through ldx_ld_pairs_dev, so nothing is ever returned inexact.
    ``r32`` holds no rounded measure: the signed correlation r of the ALT-allele indicators, unrounded float32, 4 bytes per
    pair (include/ldx.h, LDX_OUT_R32); ``r_matrix()`` turns it into blocks of the symmetric square matrix.
    """

    n_snps: int
    unit_begin: int
    unit_end: int
    ld32: Optional[torch.Tensor] = None      # float32 [(units)*1024, 2]  (r_square, d_prime) rounded to 4 dp
    raw: Optional[torch.Tensor] = None       # float64 [(units)*1024, 2]  unrounded
    n11: Optional[torch.Tensor] = None       # int32   [(units)*1024]     alt/alt haplotype counts
    k16: Optional[torch.Tensor] = None       # int16   [(units)*1024, 2]  bit patterns of the uint16 cells
    panel: Optional[PackedPanel] = None      # the panel the result came from (resolves escape cells)
    k16one: Optional[torch.Tensor] = None    # int16   [(units)*1024]     one measure's uint16 cells (fmt k16r / k16d)
    one_fmt: Optional[str] = None            # "k16r" / "k16d" when k16one is set
    r32: Optional[torch.Tensor] = None       # float32 [(units)*1024]     signed r (fmt r32)
    ws: Optional[torch.Tensor] = None        # the matrix kernel's pass-scheduler workspace (include/ldx.h, ldx_triangle_ex_dev):
                                             # zeroed once here, re-armed by every launch; one per result buffer, because two
                                             # launches that may overlap write different buffers
    dosage: bool = False                     # r32 only: the cells are genotype-dosage r (ld_triangle(dosage=True))

    @property
    def fmt(self) -> str:
        if self.r32 is not None:
            return "r32"
        if self.k16one is not None:
            return self.one_fmt
        return "ld32" if self.ld32 is not None else "k16"

    @property
    def cells(self) -> torch.Tensor:
        if self.r32 is not None:
            return self.r32
        if self.k16one is not None:
            return self.k16one
        return self.ld32 if self.ld32 is not None else self.k16

    def cell_index(self, rows, cols) -> np.ndarray:
        """Flat element index (relative to this shard) of cells (row > col)."""
        rows = np.asarray(rows, dtype=np.int64)
        cols = np.asarray(cols, dtype=np.int64)
        if np.any(rows <= cols):
            raise ValueError("cell_index needs row > col")
        npad = lib.ldx_padded_snps(self.n_snps)
        G = npad // 8
        t = cols // 128
        g = rows // 8
        u = t * G - 8 * t * (t - 1) + (g - 16 * t)
        return (u - self.unit_begin) * UNIT_PAIRS + _lib.cell_offset(rows % 8, cols % 128, self.fmt)

    def k_and_int0(self, idx) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(k int64 [m, 2], int0 bool [m, 2], escape bool [m, 2]) of the cells at flat indices ``idx`` (host arrays);
        k of an escape cell is -1."""
        self._rounded_only("k_and_int0")
        ix = torch.as_tensor(np.asarray(idx, dtype=np.int64), device=self.cells.device)
        if self.k16one is not None:          # one measure: arrays of shape [m, 1]
            u = self.k16one[ix].cpu().numpy().view(np.uint16).astype(np.int64).reshape(-1, 1)
            int0 = (u & _lib.K16_INT0) != 0
            esc = u == _lib.K16_BIG
            return np.where(esc, -1, np.where(int0, 0, u)), int0, esc
        if self.ld32 is not None:
            v = self.ld32[ix].cpu().numpy()
            esc = np.isnan(v)
            k = np.where(esc, -1, np.rint(np.nan_to_num(v).astype(np.float64) * 1e4)).astype(np.int64)
            return k, np.signbit(v) & (v == 0), esc
        u = self.k16[ix].cpu().numpy().view(np.uint16).astype(np.int64)
        int0 = (u & _lib.K16_INT0) != 0
        esc = u == _lib.K16_BIG
        return np.where(esc, -1, np.where(int0, 0, u)), int0, esc

    def dense(self, measure: str = "r_square", thres: Optional[float] = None,
              rows: Optional[Tuple[int, int]] = None) -> torch.Tensor:
        """ld_two_dim of ld_triangle.py:114,223-230 as float32 [rows][n_snps] on the device.

        Cells the reference leaves at the template's int 0 (row <= col, or rounded measure below
        ``thres``) hold -0.0; a computed int 0 (monomorphic variant) is -0.0 too, a float 0.0 is +0.0.
        Escape cells come out as NaN (``dense_values`` resolves them).  Needs the full triangle.
        """
        self._rounded_only("dense")
        if not self.unsharded:
            raise _lib.LdxError("dense() needs an unsharded TriangleResult")
        if self.k16one is not None and _lib.ONE_MEASURE[self.one_fmt] != measure:
            raise _lib.LdxError(f"this result holds {_lib.ONE_MEASURE[self.one_fmt]} only (format {self.one_fmt})")
        r0, r1 = rows if rows is not None else (0, self.n_snps)
        out = torch.empty((r1 - r0, self.n_snps), dtype=torch.float32, device=self.cells.device)
        check(lib.ldx_triangle_dense_ex_dev(self.cells.data_ptr(), _lib.FORMATS[self.fmt], self.n_snps,
                                            MEASURES[measure], 0 if thres is None else 1,
                                            0.0 if thres is None else float(thres), r0, r1, out.data_ptr(),
                                            self.n_snps, _stream_ptr()), "ldx_triangle_dense_ex_dev")
        return out

    def dense_values(self, measure: str = "r_square", thres: Optional[float] = None,
                     rows: Optional[Tuple[int, int]] = None):
        """``dense`` on the host plus the exact values of its escape cells: (float32 array [rows][n_snps],
        {(row, col): Python value}).  The dict holds, for every NaN cell of the array, what the reference's
        ld_two_dim holds there: round(x, 4) as a float, or the int 0 when it lies below ``thres``
        (ld_triangle.py:223-230)."""
        self._rounded_only("dense_values")
        r0, _ = rows if rows is not None else (0, self.n_snps)
        d = self.dense(measure, thres, rows).cpu().numpy()
        rr, cc = np.nonzero(np.isnan(d))
        fixes = {}
        if rr.size:
            if self.panel is None:
                raise _lib.LdxError("escape cells need the panel (TriangleResult.panel) to be resolved")
            ex = ld_pairs(self.panel, rr + r0, cc)
            col = 0 if measure == "r_square" else 1
            for a, b, k in zip((rr + r0).tolist(), cc.tolist(), ex["k"][:, col].tolist()):
                v = k / 10000.0
                fixes[(a, b)] = 0 if (thres is not None and v < thres) else v
        return d, fixes

    @property
    def unsharded(self) -> bool:
        return self.unit_begin == 0 and self.unit_end == lib.ldx_triangle_units(self.n_snps)

    def _rounded_only(self, what: str) -> None:
        if self.r32 is not None:
            raise _lib.LdxError(f"{what}() reads a rounded measure; an r32 result holds signed r (use r_matrix())")

    def r_matrix(self, rows: Optional[Tuple[int, int]] = None, cols: Optional[Tuple[int, int]] = None) -> torch.Tensor:
        """Block [rows[0], rows[1]) x [cols[0], cols[1]) (default: everything) of the symmetric square matrix of signed r, as a
        float32 device tensor: (i, j) and (j, i) both hold the strip cell of max(i, j), min(i, j); the diagonal is
        (n - a_i) / r_i -- 1.0 for a polymorphic SNP without missing codes, -0.0 for a degenerate one
        (ldx_triangle_r_block_dev).  A dosage result has its own diagonal: 1.0 where the dosage has variance (v_i > 0), -0.0
        otherwise (ldx_triangle_r_block_dosage_dev).  Needs an unsharded r32 result."""
        if self.r32 is None:
            raise _lib.LdxError(f"r_matrix() needs an r32 result (this one is {self.fmt})")
        if not self.unsharded:
            raise _lib.LdxError("r_matrix() needs an unsharded TriangleResult")
        if self.panel is None:
            raise _lib.LdxError("r_matrix() needs the panel (TriangleResult.panel) for the diagonal")
        n = self.n_snps
        r0, r1 = rows if rows is not None else (0, n)
        c0, c1 = cols if cols is not None else (0, n)
        if not (0 <= r0 <= r1 <= n and 0 <= c0 <= c1 <= n):
            raise _lib.LdxError(f"r_matrix(): block {rows} x {cols} outside the {n} x {n} matrix")
        out = torch.empty((r1 - r0, c1 - c0), dtype=torch.float32, device=self.r32.device)
        if out.numel():
            p = self.panel
            if self.dosage:
                check(lib.ldx_triangle_r_block_dosage_dev(self.r32.data_ptr(), n, p.dosage_stats()[1].data_ptr(), r0, r1, c0, c1,
                                                          out.data_ptr(), c1 - c0, _stream_ptr()),
                      "ldx_triangle_r_block_dosage_dev")
                return out
            check(lib.ldx_triangle_r_block_dev(self.r32.data_ptr(), n, p.acnt.data_ptr(), p.rcnt.data_ptr(), p.n_hap,
                                               r0, r1, c0, c1, out.data_ptr(), c1 - c0, _stream_ptr()),
                  "ldx_triangle_r_block_dev")
        return out


def ld_triangle(panel: PackedPanel, unit_range: Optional[Tuple[int, int]] = None, want_raw: bool = False,
                want_n11: bool = False, out: Optional[TriangleResult] = None, fmt: str = "ld32",
                path: Optional[str] = None, dosage: bool = False) -> TriangleResult:
    """All row > col pairs of the panel: var_1 = row, var_2 = col (ld_triangle.py:193-194).

    ``dosage=True`` (with ``fmt='r32'`` and the whole triangle only): the cells are the genotype-dosage correlation -- r of
    the ALT dosages 0 / 1 / 2 of the n_hap / 2 individuals (haplotypes 2k and 2k + 1), which does not depend on phase: PLINK's
    and LDSC's r (include/ldx.h, ldx_triangle_dosage_dev).  It runs on the FP4 kernel only.

    ``unit_range`` restricts the work to a contiguous slice of the unit list (multi-GPU sharding);
    ``out`` re-uses the buffers of a previous result of the same shape (benchmark loops); ``fmt`` picks the cell
    format ('ld32': 8 bytes per pair, 'k16': 4 bytes per pair, 'k16r' / 'k16d': ONE measure, 2 bytes per pair -- the kernel
    then skips the other value's arithmetic; 'r32': signed r, unrounded float32, 4 bytes per pair); ``path`` overrides the process-wide kernel choice ('fp4', 'mfma', 'popcount')
    for this call.
    """
    total = panel.n_units
    u0, u1 = (0, total) if unit_range is None else unit_range
    u0, u1 = max(0, u0), min(total, u1)
    cells = max(0, u1 - u0) * UNIT_PAIRS
    dev = panel.device
    if fmt not in _lib.FORMATS:
        raise _lib.LdxError(f"unknown cell format {fmt!r}")
    if fmt != "ld32" and want_raw:
        raise _lib.LdxError("the unrounded output travels with the ld32 format only")
    if fmt in _lib.ONE_MEASURE and want_n11:
        raise _lib.LdxError("the one-measure formats take no side output")
    if fmt == "r32" and want_n11:
        raise _lib.LdxError("the r32 format takes no side output")
    if dosage:
        if fmt != "r32":
            raise _lib.LdxError(f"ld_triangle: dosage=True needs fmt='r32' (got {fmt!r}): the rounded measures are haplotype statistics")
        if unit_range is not None:
            raise _lib.LdxError("ld_triangle: dosage=True does not take unit_range (no sharded dosage triangle)")
        if panel.n_hap % 2:
            raise _lib.LdxError(f"ld_triangle: dosage=True needs an even n_hap (got {panel.n_hap}): individual k owns haplotypes 2k and 2k + 1")
    if out is not None and out.dosage != bool(dosage):
        raise _lib.LdxError("ld_triangle: `out` was made with another `dosage`")
    if out is None:
        out = TriangleResult(panel.n_snps, u0, u1,
                             torch.empty((cells, 2), dtype=torch.float32, device=dev) if fmt == "ld32" else None,
                             torch.empty((cells, 2), dtype=torch.float64, device=dev) if want_raw else None,
                             torch.empty(cells, dtype=torch.int32, device=dev) if want_n11 else None,
                             torch.empty((cells, 2), dtype=torch.int16, device=dev) if fmt == "k16" else None,
                             k16one=torch.empty(cells, dtype=torch.int16, device=dev) if fmt in _lib.ONE_MEASURE else None,
                             one_fmt=fmt if fmt in _lib.ONE_MEASURE else None,
                             r32=torch.empty(cells, dtype=torch.float32, device=dev) if fmt == "r32" else None,
                             dosage=bool(dosage))
    elif (out.n_snps, out.unit_begin, out.unit_end, out.fmt) != (panel.n_snps, u0, u1, fmt):
        raise _lib.LdxError("ld_triangle: `out` has a different shape or format")
    out.panel = panel
    if cells:
        pcode = lib.ldx_get_triangle_path() if path is None else PATHS[path]
        if out.ws is None and pcode != PATHS["popcount"]:
            out.ws = torch.zeros(lib.ldx_triangle_workspace_bytes(), dtype=torch.uint8, device=dev)
        if dosage:
            check(lib.ldx_triangle_dosage_dev(*_dosage_panel(panel), panel.n_snps, panel.n_hap, u0, u1, pcode,
                                              out.r32.data_ptr(), _ptr(out.ws), 0 if out.ws is None else out.ws.numel(),
                                              _stream_ptr()), "ldx_triangle_dosage_dev")
            return out
        check(lib.ldx_triangle_ex_dev(panel.alt.data_ptr(), panel.fa.data_ptr(), panel.fr.data_ptr(),
                                      panel.q.data_ptr(), panel.n_snps, panel.n_hap, u0, u1, pcode,
                                      _lib.FORMATS[fmt], out.cells.data_ptr(), _ptr(out.raw), _ptr(out.n11),
                                      _ptr(out.ws), 0 if out.ws is None else out.ws.numel(), _stream_ptr()),
              "ldx_triangle_ex_dev")
    return out


# --------------------------------------------------------------------------- n11 block / epilogue / explicit pairs
def pair_counts(panel_i: PackedPanel, panel_j: Optional[PackedPanel] = None) -> torch.Tensor:
    """n11[i][j] = #haplotypes with code 1 at SNP i of panel_i and SNP j of panel_j (calc_ld.py:32)."""
    pj = panel_j or panel_i
    if pj.n_hap != panel_i.n_hap:
        raise _lib.LdxError("pair_counts: panels differ in haplotype count")
    out = torch.empty((panel_i.n_snps, pj.n_snps), dtype=torch.int32, device=panel_i.device)
    check(lib.ldx_pair_counts_dev(panel_i.alt.data_ptr(), panel_i.n_snps, pj.alt.data_ptr(), pj.n_snps,
                                  panel_i.n_hap, out.data_ptr(), pj.n_snps, _stream_ptr()),
          "ldx_pair_counts_dev")
    return out


def ld_pairs(panel: PackedPanel, rows, cols) -> dict:
    """calc_ld for an explicit list of pairs (var_1 = rows[p], var_2 = cols[p]) of one panel, exact for any magnitude:
    host arrays ``k`` (float64 [m, 2]: round(x, 4) * 10^4 of r_square, d_prime), ``raw`` (float64 [m, 2]), ``flags``
    (uint8, LDX_FLAG_*: which value is the reference's int 0) and ``n11`` (uint32)."""
    dev = panel.device
    r = torch.as_tensor(np.ascontiguousarray(np.asarray(rows, dtype=np.int64).astype(np.int32))).to(dev)
    c = torch.as_tensor(np.ascontiguousarray(np.asarray(cols, dtype=np.int64).astype(np.int32))).to(dev)
    m = int(r.numel())
    if int(c.numel()) != m:
        raise _lib.LdxError("ld_pairs: rows and cols differ in length")
    k = torch.empty((m, 2), dtype=torch.float64, device=dev)
    raw = torch.empty((m, 2), dtype=torch.float64, device=dev)
    flags = torch.empty(m, dtype=torch.uint8, device=dev)
    n11 = torch.empty(m, dtype=torch.int32, device=dev)
    if m:
        check(lib.ldx_ld_pairs_dev(panel.alt.data_ptr(), panel.acnt.data_ptr(), panel.rcnt.data_ptr(), panel.n_snps,
                                   panel.n_hap, r.data_ptr(), c.data_ptr(), m, k.data_ptr(), raw.data_ptr(),
                                   flags.data_ptr(), n11.data_ptr(), _stream_ptr()), "ldx_ld_pairs_dev")
    return {"k": k.cpu().numpy(), "raw": raw.cpu().numpy(), "flags": flags.cpu().numpy(),
            "n11": n11.cpu().numpy().view(np.uint32)}


def ld_from_counts(n: int, n11, a1, r1, a2, r2, device: Optional[torch.device] = None, full: bool = False):
    """The epilogue alone (calc_ld.py:33-97) on arrays of counts.

    Returns (raw float64 [m,2], rounded float32 [m,2], flags uint8 [m]) as device tensors; with ``full`` also
    k (float64 [m,2]: round(x, 4) * 10^4, exact for any magnitude), the 4-byte cells (int16 [m,2], the bit patterns
    of ldx_k16) and a bool [m] telling which pairs the fp32 epilogue tier would have kept (the others go to fp64).
    """
    dev = device or torch.device("cuda", torch.cuda.current_device())
    def up(x):
        t = torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.uint32)).view(np.int32))
        return t.to(dev)
    t11, ta1, tr1, ta2, tr2 = (up(x) for x in (n11, a1, r1, a2, r2))
    m = t11.numel()
    raw = torch.empty((m, 2), dtype=torch.float64, device=dev)
    rnd = torch.empty((m, 2), dtype=torch.float32, device=dev)
    flags = torch.empty(m, dtype=torch.uint8, device=dev)
    k = torch.empty((m, 2), dtype=torch.float64, device=dev) if full else None
    k16 = torch.empty((m, 2), dtype=torch.int16, device=dev) if full else None
    check(lib.ldx_ld_from_counts_ex_dev(int(n), m, t11.data_ptr(), ta1.data_ptr(), tr1.data_ptr(), ta2.data_ptr(),
                                        tr2.data_ptr(), raw.data_ptr(), _ptr(k), rnd.data_ptr(), _ptr(k16),
                                        flags.data_ptr(), _stream_ptr()), "ldx_ld_from_counts_ex_dev")
    sure32 = (flags & 0x80) != 0       # LDX_FLAG_F32_SURE: the fp32 epilogue tier would have kept the pair
    flags = flags & 3
    if full:
        return raw, rnd, flags, k, k16, sure32
    return raw, rnd, flags


# --------------------------------------------------------------------------- area
class AreaHits:
    """Thresholded hits of a windowed scan, sorted by (query row, opposing row) = VCF order."""

    def __init__(self, query: torch.Tensor, oppos: torch.Tensor, ld32: torch.Tensor, n_pairs, offsets=None,
                 band_passes=None):
        self.query = query        # int64 [n]  panel row of var_1 (the query)
        self.oppos = oppos        # int64 [n]  panel row of var_2 (the opposing variant)
        self.ld32 = ld32          # float32 [n, 2]  rounded (r_square, d_prime), -0.0 = int 0
        self._n_pairs = n_pairs   # int, or a callable that counts on first use (bookkeeping only)
        self.offsets = offsets    # int32 [n_snps + 1] (device): the hits of query row q are [offsets[q], offsets[q + 1])
        self._band_passes = band_passes

    @property
    def n_pairs(self) -> int:
        """(query, opposing) pairs inside the windows that were evaluated."""
        if callable(self._n_pairs):
            self._n_pairs = self._n_pairs()
        return self._n_pairs

    @property
    def band_passes(self) -> Optional[int]:
        """Passes (4 units of 64 rows x 128 columns) the matrix-pipe band evaluated for this call; None for the popcount
        scan.  Instrumentation: shows how the work of a sharded scan splits."""
        if callable(self._band_passes):
            self._band_passes = self._band_passes()
        return self._band_passes

    def __len__(self) -> int:
        return int(self.query.numel())

    def python_values(self, panel: PackedPanel):
        """[(r_square, d_prime)] per hit as the reference's Python values (float round(x, 4), or the int 0).  Hits whose
        float32 is the escape NaN (a value >= 1024: only with missing codes) are resolved exactly through ld_pairs."""
        v = self.ld32.cpu().numpy().reshape(-1, 2)
        esc = np.isnan(v)
        k = np.rint(np.where(esc, 0, v).astype(np.float64) * 1e4)
        int0 = np.signbit(v) & (v == 0)
        out = [[0 if z else kk / 10000.0 for kk, z in zip(kr.tolist(), zr.tolist())] for kr, zr in zip(k, int0)]
        rows = np.flatnonzero(esc.any(axis=1))
        if rows.size:
            ex = ld_pairs(panel, self.query.cpu().numpy()[rows], self.oppos.cpu().numpy()[rows])
            for r, kk in zip(rows.tolist(), ex["k"]):
                for c in (0, 1):
                    if esc[r, c]:
                        out[r][c] = float(kk[c]) / 10000.0
        return [tuple(x) for x in out]


class _AreaPlan:
    """Buffers of one ld_area call shape (panel, positions tensor, queries, flank, measure, threshold) and -- once the
    shape has been seen twice -- the HIP graph of its launches (query mask, band plan, scan, offsets, scatter, ordering:
    ten small launches around one 0.36 ms kernel, launch-bound when issued one by one)."""

    def __init__(self, panel, nq, cap):
        dev = panel.device
        self.cap = cap
        self.ws_bytes = lib.ldx_area_workspace_bytes(panel.n_snps, panel.n_hap, nq)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.fin_bytes = lib.ldx_area_finish_workspace_bytes(panel.n_snps)
        self.fin = torch.empty(self.fin_bytes, dtype=torch.uint8, device=dev)
        self.n_hits = torch.zeros(1, dtype=torch.int64, device=dev)
        self.summary = torch.zeros(2, dtype=torch.int64, device=dev)
        self.offsets = torch.empty(panel.n_snps + 1, dtype=torch.int32, device=dev)
        self.raw = torch.empty((cap, 4), dtype=torch.int32, device=dev)      # ldx_hit = {u32, u32, f32, f32}
        self.hits = torch.empty((cap, 4), dtype=torch.int32, device=dev)
        self.graph = None
        self.uses = 0
        self.nbytes = sum(int(t.numel()) * t.element_size() for t in (self.ws, self.fin, self.raw, self.hits, self.offsets))


_PLAN_BYTES_MAX = 1 << 30      # kept ld_area plans per panel (buffers a plan pins while it is kept)


def _area_launch(panel, pos, q, nq, flank, measure, thres, plan, events=None):
    """The launches of one scan + finish on torch's current stream (no host synchronisation)."""
    if events is not None:
        del events[:]
        events.extend(torch.cuda.Event(enable_timing=True) for _ in range(3))
        events[0].record()
    counts = lib.ldx_area_finish_counts(plan.fin.data_ptr())     # the scan counts per query row as it stores the hits
    check(lib.ldx_area_scan_dev(panel.alt.data_ptr(), panel.fa.data_ptr(), panel.fr.data_ptr(), panel.q.data_ptr(),
                                panel.n_snps, panel.n_hap, pos.data_ptr(), q.data_ptr(), nq, int(flank),
                                MEASURES[measure], float(thres), plan.raw.data_ptr(), plan.cap, plan.n_hits.data_ptr(),
                                counts, plan.ws.data_ptr(), plan.ws_bytes, _stream_ptr()), "ldx_area_scan_dev")
    if events is not None:
        events[1].record()
    check(lib.ldx_area_finish_ex_dev(plan.raw.data_ptr(), plan.n_hits.data_ptr(), plan.cap, panel.n_snps,
                                     plan.hits.data_ptr(), plan.offsets.data_ptr(), plan.summary.data_ptr(),
                                     plan.fin.data_ptr(), plan.fin_bytes, 1, _stream_ptr()), "ldx_area_finish_ex_dev")
    if events is not None:
        events[2].record()


def ld_area(panel: PackedPanel, positions, queries: Optional[Sequence[int]] = None, flank: int = 100000,
            measure: str = "r_square", thres: float = 0.8, hit_capacity: Optional[int] = None,
            check_positions: bool = True, events: Optional[list] = None, use_graph: Optional[bool] = None) -> AreaHits:
    """Windowed scan of ld_area.py:152-276 over the panel.

    positions: ascending 1-based coordinates of the panel's SNPs (VCF order).  queries: panel
    row indices of the query variants (default: every SNP).  For each query q the opposing
    variants are o != q with max(0, pos_q - flank) < pos_o <= pos_q + flank (pysam's fetch,
    ld_area.py:174-177,215-217); var_1 = query, var_2 = opposing; kept when the rounded
    ``measure`` >= thres (ld_area.py:248).

    Everything up to the ordered hit list runs on the device (scan, which counts per query as it stores -> exclusive scan
    -> scatter -> per-query order: ldx_area_scan_dev + ldx_area_finish_ex_dev); the host reads two integers at the end
    to size the result.  When the same scan shape comes again -- the same panel, the same DEVICE tensor of positions,
    the same queries / flank / measure / threshold: a driver walking tables of one chromosome -- its launches are
    replayed as ONE HIP graph from the second repetition on (``use_graph``: None = that rule, False = never, True = from the
    first call); the plan (buffers + graph) lives on the panel and keeps its buffers resident until it is evicted (eight
    shapes / 1 GiB per panel) or ``panel.clear_area_plans()`` is called.  A plan's graph carries its own ticket counters
    (in the plan's workspace), so plans of different panels or shapes may be replayed on different streams at once; one
    plan is one set of buffers -- the SAME shape on the same panel from two threads at once is the caller's to serialise.
    ``events`` (instrumentation, bench.py): a list that receives three torch events of the current stream -- before the
    scan, between the scan and the finishing kernels, after them; forces eager launches.
    """
    dev = panel.device
    pos_key = None
    if isinstance(positions, torch.Tensor):
        pos = positions.to(dev, dtype=torch.int64).contiguous()
        if pos.data_ptr() == positions.data_ptr():
            pos_key = (pos.data_ptr(), int(pos.numel()))
        # a device tensor is checked on the device (one more host round trip); callers that scan one chromosome many
        # times pass check_positions=False after the first call
        if check_positions and pos.numel() > 1 and bool((pos[1:] < pos[:-1]).any().item()):
            raise _lib.LdxError("positions must ascend (VCF order): the window search is a binary search")
    else:
        pos_h = np.ascontiguousarray(np.asarray(positions, dtype=np.int64))
        if pos_h.size > 1 and bool((pos_h[1:] < pos_h[:-1]).any()):
            raise _lib.LdxError("positions must ascend (VCF order): the window search is a binary search")
        pos = torch.as_tensor(pos_h).to(dev)
    if pos.numel() != panel.n_snps:
        raise _lib.LdxError("positions must have one entry per SNP")
    plans = panel.__dict__.setdefault("_area_plans", {})
    q_key = None
    if queries is None:
        q = plans.get("all_rows")
        if q is None:
            q = plans["all_rows"] = torch.arange(panel.n_snps, dtype=torch.int32, device=dev)
        q_key = "all"
    else:
        # the kernels want STRICTLY ascending rows (include/ldx.h): a repeated query is one query -- the reference would write
        # the same result file twice (ld_area.py:152-292) -- and "as many queries as SNPs" must mean every SNP once
        qn = np.unique(np.asarray(queries, dtype=np.int64))
        if qn.size == 0:
            e = torch.empty(0, dtype=torch.int64, device=dev)
            return AreaHits(e, e, torch.empty((0, 2), dtype=torch.float32, device=dev), 0,
                            torch.zeros(panel.n_snps + 1, dtype=torch.int32, device=dev))
        if qn[0] < 0 or qn[-1] >= panel.n_snps:
            raise _lib.LdxError("query row out of range")
        q = torch.as_tensor(qn.astype(np.int32)).to(dev)
    nq = int(q.numel())
    cap = int(hit_capacity) if hit_capacity is not None else max(1 << 20, 16 * nq)   # slots (16 B each); an overflow re-runs with the exact count
    # the plan of this call shape (only shapes that can come again unchanged have one that is kept)
    key = None
    if pos_key is not None and q_key is not None and events is None and use_graph is not False:
        key = (pos_key, q_key, int(flank), measure, float(thres), get_area_path(), panel.alt.data_ptr())
    plan = plans.get(key) if key is not None else None
    if plan is not None and plan.cap < cap:
        plan = None
    while True:
        if plan is None:
            plan = _AreaPlan(panel, nq, cap)
            if key is not None:
                # A kept plan pins its buffers (two hit buffers of `cap` 16-byte slots, the workspaces) and, from its second
                # use, a HIP graph: at most eight shapes and _PLAN_BYTES_MAX bytes per panel, oldest dropped first
                # (PackedPanel.clear_area_plans() drops them all).
                kept = [k for k in plans if k != "all_rows"]
                while kept and (len(kept) >= 8 or sum(plans[k].nbytes for k in kept) + plan.nbytes > _PLAN_BYTES_MAX):
                    del plans[kept.pop(0)]
                plans[key] = plan
        plan.uses += 1
        if key is not None and plan.graph is None and (use_graph or plan.uses >= 2) and \
                not torch.cuda.is_current_stream_capturing():
            try:                                    # capture the launches once; a failure leaves the eager path
                torch.cuda.current_stream().synchronize()   # this stream's launches are done (torch's graph context then
                                                            # synchronises the device once more, on every capture: its own rule)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):   # other threads (the shells' table workers) keep allocating
                    _area_launch(panel, pos, q, nq, flank, measure, thres, plan)
                plan.graph = g
            except Exception:                       # noqa: BLE001
                plan.graph = False
                torch.cuda.synchronize()
        if plan.graph:
            plan.graph.replay()
        else:
            _area_launch(panel, pos, q, nq, flank, measure, thres, plan, events)
        total, reserved = (int(x) for x in plan.summary.tolist())             # the one host round trip
        if reserved <= plan.cap:
            break
        cap = reserved + 4096            # the count is exact for a re-run: one retry suffices
        if key is not None:
            plans.pop(key, None)
        plan = None
    # the caller's copy of the result -- query / opposing rows as int64, the value pairs, and for a kept plan (whose buffers
    # the next call overwrites) the offsets index and the band's pass count -- in ONE launch (ldx_area_results_dev; it was
    # five small torch kernels, ~20 us of a 0.39 ms call)
    qrow = torch.empty(total, dtype=torch.int64, device=dev)
    orow = torch.empty(total, dtype=torch.int64, device=dev)
    ld32 = torch.empty((total, 2), dtype=torch.float32, device=dev)
    offsets = torch.empty_like(plan.offsets) if key is not None else plan.offsets
    use_band = get_area_path() != "popcount" and (get_area_path() != "auto" or (nq * 16 >= panel.n_snps and panel.n_snps >= 2))
    word = None
    if use_band:
        off = lib.ldx_area_band_passes_offset(panel.n_snps)
        word_src = plan.ws[off:off + 4]
        word = torch.empty(4, dtype=torch.uint8, device=dev) if key is not None else word_src
    check(lib.ldx_area_results_dev(plan.hits.data_ptr(), total, qrow.data_ptr(), orow.data_ptr(), ld32.data_ptr(),
                                   plan.offsets.data_ptr(), offsets.data_ptr() if key is not None else None,
                                   panel.n_snps + 1,
                                   word_src.data_ptr() if (use_band and key is not None) else None,
                                   word.data_ptr() if (use_band and key is not None) else None, _stream_ptr()),
          "ldx_area_results_dev")

    def count_pairs() -> int:
        # pairs evaluated = sum over queries of window population (bookkeeping, on device, only when asked for)
        qpos = pos[q.to(torch.int64)]
        lo = torch.searchsorted(pos, torch.clamp(qpos - flank, min=0), right=True)
        hi = torch.searchsorted(pos, qpos + flank, right=True)
        self_in = torch.clamp(qpos - flank, min=0) < qpos      # the query lies in its own window unless flank == 0
        return int((hi - lo).sum().item()) - int(self_in.sum().item())

    band = None
    if use_band:
        band = lambda: int(word.view(torch.int32).item())    # noqa: E731
    return AreaHits(qrow, orow, ld32, count_pairs, offsets, band)


# --------------------------------------------------------------------------- genotype dosage
def dosage_host(codes) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Host mirror of ldx_dosage_stats_dev (include/ldx.h) in pure numpy: ``(a, hom, v)`` int64 [n_snps] from an allele-code
    matrix [n_snps][n_hap], n_hap even.  Individual k owns haplotypes 2k and 2k + 1; its dosage g counts code 1 ONLY (REF,
    missing and any other allele count 0); a = sum g, hom = #{g == 2}, v = N (a + 2 hom) - a^2 with N = n_hap / 2 -- N^2 times
    the variance of g, 0 exactly for the SNPs the dosage operators treat as degenerate."""
    c = np.asarray(codes)
    if c.ndim != 2 or c.shape[1] % 2:
        raise _lib.LdxError(f"dosage_host: codes must be [n_snps][n_hap] with an even n_hap, got shape {c.shape}")
    alt = (c == 1)
    g = alt[:, 0::2].astype(np.int64) + alt[:, 1::2].astype(np.int64)
    a = g.sum(axis=1)
    hom = (g == 2).sum(axis=1)
    n_ind = c.shape[1] // 2
    return a, hom, n_ind * (a + 2 * hom) - a * a


def _dosage_refused(what: str, dosage) -> None:
    """The operators without a dosage form refuse the flag: none of them may silently compute haplotype r."""
    if dosage:
        raise _lib.LdxError(f"{what}: no genotype-dosage form (dosage=True is available for ld_triangle(fmt='r32'), ld_score, "
                            "ld_neighbors, ld_prune and ld_clump)")


def _dosage_check(what: str, panel: PackedPanel, regions=None) -> None:
    """Argument rules of the dosage operators, checked before anything touches the device."""
    if regions is not None:
        raise _lib.LdxError(f"{what}: regions= together with dosage=True is not available")
    if panel.n_hap % 2:
        raise _lib.LdxError(f"{what}: dosage=True needs an even n_hap (got {panel.n_hap}): individual k owns haplotypes 2k and 2k + 1")


# --------------------------------------------------------------------------- LD scores
SCORE_SCALE = float(1 << 32)    # sums are integers in units of 2^-32 r^2 (include/ldx.h, ldx_ld_score_dev)
MAX_ANNOT = 8


def score_terms(r) -> np.ndarray:
    """Host mirror of the kernel's term (include/ldx.h, ldx_ld_score_dev): rint(2^32 * (r *f32 r)) as uint64, from float32 r
    cells (ld_triangle(fmt="r32") / TriangleResult.r_matrix()).  One float32 multiply, then exact scaling and round-half-even."""
    r = np.asarray(r, dtype=np.float32)
    r2 = np.multiply(r, r, dtype=np.float32)
    return np.rint(np.ldexp(r2.astype(np.float64), 32)).astype(np.uint64)


def window_bounds(positions, window: int) -> Tuple[np.ndarray, np.ndarray]:
    """[lo, hi) row range of every SNP's window |pos_i - pos_j| <= window over non-decreasing positions."""
    pos = np.asarray(positions, dtype=np.int64)
    lo = np.searchsorted(pos, pos - window, side="left")
    hi = np.searchsorted(pos, pos + window, side="right")
    return lo, hi


def window_counts(positions, window: int, live, annot_bits=None, n_annot: int = 0) -> np.ndarray:
    """m of LDSC: int64 [n, 1 + n_annot], the number of SNPs j with |pos_i - pos_j| <= window (i itself included) that are
    `live` (not degenerate) and -- column 1 + k -- carry bit k of annot_bits[j]."""
    lo, hi = window_bounds(positions, window)
    live = np.asarray(live, dtype=bool)
    cols = [live]
    if n_annot:
        bits = np.asarray(annot_bits, dtype=np.uint8)
        cols += [live & (((bits >> k) & 1) != 0) for k in range(n_annot)]
    ind = np.stack(cols, axis=1).astype(np.int64)
    pre = np.concatenate([np.zeros((1, ind.shape[1]), dtype=np.int64), np.cumsum(ind, axis=0)])
    return pre[hi] - pre[lo]


def adjust_l2(l2, m, n_obs: int) -> np.ndarray:
    """LDSC's unbiased r^2, r^2 - (1 - r^2) / (n_obs - 2), summed over a window: linear in r^2, so it applies to the sums
    as (n_obs - 1) / (n_obs - 2) * L - m / (n_obs - 2) with m the number of terms (window_counts)."""
    if n_obs <= 2:
        raise _lib.LdxError("adjusted() needs n_obs > 2")
    return (n_obs - 1) / (n_obs - 2) * np.asarray(l2, dtype=np.float64) - np.asarray(m, dtype=np.float64) / (n_obs - 2)


def pack_annot(annot, n_snps: int) -> Tuple[np.ndarray, int]:
    """bool / 0-1 array [n, K] (or [n] for K = 1), K <= 8 -> (uint8 bitmask per SNP, K)."""
    a = np.asarray(annot)
    if a.ndim == 1:
        a = a[:, None]
    if a.ndim != 2 or a.shape[0] != n_snps:
        raise _lib.LdxError(f"annot must have shape [n_snps, K] (n_snps = {n_snps}), got {a.shape}")
    k = a.shape[1]
    if k > MAX_ANNOT:
        raise _lib.LdxError(f"at most {MAX_ANNOT} annotation categories (got {k})")
    if a.dtype != bool and not np.isin(a, (0, 1)).all():
        raise _lib.LdxError("annot must be boolean or 0/1")
    ab = a.astype(bool)
    bits = np.zeros(n_snps, dtype=np.uint8)
    for j in range(k):
        bits |= (ab[:, j].astype(np.uint8) << j)
    return bits, k


@dataclass
class LDScores:
    """LD scores of one panel (ld_score).  ``sums`` is the device uint64 tensor [n, 1 + K] the kernel wrote (units of 2^-32
    r^2); ``l2`` (float64 [n, 1 + K]) = sums / 2^32 and ``m`` (int64 [n, 1 + K]: non-degenerate SNPs in each window and
    category, self included) are computed on the host when first asked for."""

    sums: torch.Tensor
    positions: np.ndarray
    window: int
    n_hap: int
    annot_bits: Optional[np.ndarray]
    n_annot: int
    panel: Optional[PackedPanel] = None
    _l2: Optional[np.ndarray] = None
    _m: Optional[np.ndarray] = None
    _live: Optional[np.ndarray] = None
    dosage: bool = False                     # the sums are over genotype-dosage r (ld_score(dosage=True))
    missing: Optional[str] = None            # "pairwise": the sums are over pairwise-complete r (ld_score(missing="pairwise"))

    @property
    def live(self) -> np.ndarray:
        """bool [n]: the SNP is not degenerate (a r > 0: it has ALT and REF codes; a dosage result: v > 0, the dosage varies
        among the individuals; a pairwise-complete dosage result: it varies among the individuals called at the SNP)."""
        if self._live is None and self.missing is not None:
            self._live = pw_snp_stats(self.panel, self.dosage)[1].cpu().numpy().astype(bool)
        if self._live is None and self.dosage:
            self._live = self.panel.dosage_live()
        if self._live is None:
            self._live = (self.panel.alt_counts().astype(np.int64) * self.panel.ref_counts().astype(np.int64)) > 0
        return self._live

    @property
    def l2(self) -> np.ndarray:
        if self._l2 is None:
            self._l2 = self.sums.cpu().numpy().astype(np.float64) / SCORE_SCALE
        return self._l2

    @property
    def m(self) -> np.ndarray:
        if self._m is None:
            pos = self.positions.cpu().numpy() if isinstance(self.positions, torch.Tensor) else self.positions
            self._m = window_counts(pos, self.window, self.live, self.annot_bits, self.n_annot)
        return self._m

    def adjusted(self, n_obs: Optional[int] = None) -> np.ndarray:
        """LDSC's unbiased r^2 estimate summed over the windows (adjust_l2), n_obs defaulting to n_hap -- for a dosage
        result to the number of individuals, n_hap / 2."""
        default = self.n_hap // 2 if self.dosage else self.n_hap
        return adjust_l2(self.l2, self.m, default if n_obs is None else int(n_obs))


def _band_positions(panel: PackedPanel, positions, window_bp, window_snps, check_positions: bool, what: str):
    """The band calls' positions and window: (device int64 positions, host copy or None, window).  ``window_snps`` counts
    the window in SNPs (positions 0 .. n-1); otherwise ``positions`` must be non-decreasing, one per SNP (a device tensor is
    checked on the device unless ``check_positions`` is False)."""
    n = panel.n_snps
    if panel.n_hap > _lib.MAX_HAPS:
        raise _lib.LdxError(f"n_hap {panel.n_hap} > LDX_MAX_HAPS {_lib.MAX_HAPS}")
    if window_snps is not None:
        window = int(window_snps)
        pos_h = np.arange(n, dtype=np.int64)
        pos = torch.arange(n, dtype=torch.int64, device=panel.device)
    else:
        window = int(window_bp)
        if positions is None:
            raise _lib.LdxError(f"{what} needs positions (or window_snps)")
        if isinstance(positions, torch.Tensor):
            pos = positions.to(panel.device, dtype=torch.int64).contiguous()
            if check_positions and pos.numel() > 1 and bool((pos[1:] < pos[:-1]).any().item()):
                raise _lib.LdxError("positions must be non-decreasing (VCF order)")
            pos_h = None
        else:
            pos_h = np.ascontiguousarray(np.asarray(positions, dtype=np.int64))
            if pos_h.size > 1 and bool((pos_h[1:] < pos_h[:-1]).any()):
                raise _lib.LdxError("positions must be non-decreasing (VCF order)")
            pos = torch.as_tensor(pos_h).to(panel.device)
        if pos.numel() != n:
            raise _lib.LdxError("positions must have one entry per SNP")
    if window < 0:
        raise _lib.LdxError("the window must be >= 0")
    return pos, pos_h, window


def ld_score(panel: PackedPanel, positions=None, window_bp: int = 1_000_000, window_snps: Optional[int] = None,
             annot=None, path: Optional[str] = None, workspace: Optional[torch.Tensor] = None,
             check_positions: bool = True, regions=None, dosage: bool = False, missing: Optional[str] = None) -> LDScores:
    """LD scores on the matrix-pipe band: for every SNP i, the sum of r^2 over the SNPs j with |pos_i - pos_j| <= window
    (i itself included), and with ``annot`` (bool / 0-1 [n, K], K <= 8) the same sum per category over the j that carry it
    (include/ldx.h, ldx_ld_score_dev).  r is the signed r of ld_triangle(fmt="r32"), bit for bit; the sums are exact
    integer sums of rint(2^32 r^2), so they are reproducible run to run.

    ``window_snps`` counts the window in SNPs instead of base pairs (positions 0 .. n-1).  ``path``: 'fp4' (default) or
    'mfma' (the int8 band: identical sums).  ``workspace``: a uint8 device tensor of ldx_ld_score_workspace_bytes() bytes to
    reuse (one per launch that may be in flight); by default one is allocated per call.  The call is stream-ordered: the
    host reads nothing until ``.l2`` / ``.m`` are asked for (a device tensor of positions is checked on the device unless
    ``check_positions`` is False).

    ``regions`` (an LDRegions or a region_of array; default None: no change): the sums run over the SNPs of i's own region
    only -- the positions go through region_positions, and ``LDScores.m`` counts over the same shifted positions.
    ``window_bp=None`` then means whole regions.

    ``dosage=True``: r is the genotype-dosage r of ld_triangle(fmt="r32", dosage=True), bit for bit -- what ldsc.py --l2 sums
    (include/ldx.h, ldx_ld_score_dosage_dev; the FP4 band only, not together with ``regions``).  ``LDScores.live`` is then
    v > 0 and ``adjusted()`` defaults to n_obs = n_hap / 2.

    ``missing="pairwise"``: r is the pairwise-complete r of ld_rect(missing="pairwise") -- every pair over the haplotypes
    (``dosage``: the individuals) called at both SNPs, as PLINK --r2 does (include/ldx.h, "pairwise-complete bands";
    ldx_ld_pw_score_dev: the FP4 band only, not together with ``regions``; ``workspace`` of ldx_ld_pw_band_workspace_bytes()
    bytes; with ``annot`` the band is walked once per column of the result).  A SNP's own term is 1 where it is polymorphic
    among its own called observations.  None: the call as it always was.
    """
    pairwise = _band_missing("ld_score", missing, path)
    if pairwise and regions is not None:
        raise _lib.LdxError('ld_score: regions= together with missing="pairwise" is not available: store the band with '
                            'ld_band(missing="pairwise") and sum its cells per region')
    if dosage:
        _dosage_check("ld_score", panel, regions)
    require_gpu()
    n = panel.n_snps
    pos, pos_h, window = _region_band(panel, positions, window_bp, window_snps, regions, check_positions, "ld_score")
    bits, k = (None, 0) if annot is None else pack_annot(annot, n)
    annot_d = torch.as_tensor(bits).to(panel.device) if k else None
    if pairwise:
        workspace = _plan_workspace(lib.ldx_ld_pw_band_workspace_bytes, panel, workspace)
        sums = torch.empty((n, 1 + k), dtype=torch.uint64, device=panel.device)
        diag, _ = pw_snp_stats(panel, dosage)
        check(lib.ldx_ld_pw_score_dev(*_pw_panel(panel, dosage), n, panel.n_hap, int(bool(dosage)), pos.data_ptr(),
                                      min(window, BAND_WINDOW_MAX), _ptr(annot_d), k, diag.data_ptr(), sums.data_ptr(),
                                      *_ws(workspace), _stream_ptr()), "ldx_ld_pw_score_dev")
        res = LDScores(sums, pos_h if pos_h is not None else pos, window, panel.n_hap, bits, k, panel, dosage=bool(dosage),
                       missing=missing)
        res._keep = (pos, annot_d, workspace, diag)
        return res
    pcode = _band_path(path)
    workspace = _band_workspace(lib.ldx_ld_score_workspace_bytes, panel, workspace)
    sums = torch.empty((n, 1 + k), dtype=torch.uint64, device=panel.device)
    if dosage:
        check(lib.ldx_ld_score_dosage_dev(*_dosage_panel(panel), n, panel.n_hap, pos.data_ptr(), window, _ptr(annot_d), k,
                                          pcode, sums.data_ptr(), *_ws(workspace), _stream_ptr()), "ldx_ld_score_dosage_dev")
    else:
        check(lib.ldx_ld_score_dev(*_phased_panel(panel), n, panel.n_hap, pos.data_ptr(), window, _ptr(annot_d), k, pcode,
                                   sums.data_ptr(), *_ws(workspace), _stream_ptr()), "ldx_ld_score_dev")
    res = LDScores(sums, pos_h, window, panel.n_hap, bits, k, panel, dosage=bool(dosage))
    if pos_h is None:   # positions stayed on the device: fetched with m
        res.positions = pos      # type: ignore[assignment]
    res._keep = (pos, annot_d, workspace)   # alive until the launch is done (stream-ordered frees would allow reuse anyway)
    return res


# --------------------------------------------------------------------------- LD decay
DECAY_WINDOW_MAX = 1 << 52      # larger windows act as 2^52 (include/ldx.h, ldx_ld_decay_dev)


def decay_bins(window: int, bin_width: int) -> int:
    """Number of bins of ldx_ld_decay_dev: min(window, 2^52) // bin_width + 1."""
    return min(int(window), DECAY_WINDOW_MAX) // int(bin_width) + 1


def decay_host(r, positions, window: int, bin_width: int, keep=None, live=None) -> Tuple[np.ndarray, np.ndarray]:
    """Host mirror of ldx_ld_decay_dev over an r32 square (TriangleResult.r_matrix()): (sums, counts), uint64 [n_bins] each.
    Pairs i > j with pos_i - pos_j <= window whose two SNPs are ``live`` (bool [n]: not degenerate; default: every SNP) and
    kept; the term is score_terms of the cell, the bin floor(d / bin_width) in integers, the sums integer sums."""
    r = np.asarray(r, dtype=np.float32)
    n = r.shape[0]
    pos = np.asarray(positions, dtype=np.int64)
    window, bin_width = min(int(window), DECAY_WINDOW_MAX), int(bin_width)
    if bin_width < 1:
        raise _lib.LdxError("bin_width must be >= 1")
    n_bins = decay_bins(window, bin_width)
    ok = np.ones(n, dtype=bool) if live is None else np.asarray(live, dtype=bool).copy()
    if keep is not None:
        ok &= np.asarray(keep, dtype=bool)
    rows, cols = np.tril_indices(n, -1)
    d = pos[rows] - pos[cols]
    sel = (d <= window) & ok[rows] & ok[cols]
    rows, cols, d = rows[sel], cols[sel], d[sel]
    b = d // bin_width
    counts = np.bincount(b, minlength=n_bins).astype(np.uint64)
    sums = np.zeros(n_bins, dtype=np.uint64)
    np.add.at(sums, b, score_terms(r[rows, cols]))
    return sums, counts


@dataclass
class LDDecay:
    """LD decay curve of one panel (ld_decay).  ``sums`` / ``counts_dev`` are the device uint64 tensors [n_bins] the kernel
    wrote (sums in units of 2^-32 r^2); bin b covers the distances [b bin_width, (b + 1) bin_width), the last bin ends at
    ``window``.  The host arrays are fetched when first asked for."""

    sums: torch.Tensor
    counts_dev: torch.Tensor
    bin_width: int
    window: int
    n_hap: int
    _counts: Optional[np.ndarray] = None
    _sum_r2: Optional[np.ndarray] = None

    @property
    def n_bins(self) -> int:
        return int(self.sums.numel()) if self._counts is None else int(self._counts.size)

    @property
    def counts(self) -> np.ndarray:
        """int64 [n_bins]: pairs per bin."""
        if self._counts is None:
            self._counts = self.counts_dev.cpu().numpy().astype(np.int64)
        return self._counts

    @property
    def sum_r2(self) -> np.ndarray:
        """float64 [n_bins]: sum of r^2 per bin (sums / 2^32)."""
        if self._sum_r2 is None:
            self._sum_r2 = self.sums.cpu().numpy().astype(np.float64) / SCORE_SCALE
        return self._sum_r2

    @property
    def mean_r2(self) -> np.ndarray:
        """float64 [n_bins]: mean r^2 per bin, NaN for an empty bin."""
        c = self.counts
        return np.where(c > 0, self.sum_r2 / np.maximum(c, 1), np.nan)

    @property
    def distance(self) -> np.ndarray:
        """int64 [n_bins]: the start of every bin."""
        return np.arange(self.n_bins, dtype=np.int64) * self.bin_width

    def adjusted(self, n_obs: Optional[int] = None) -> np.ndarray:
        """LDSC's unbiased estimate of the mean, (n - 1) / (n - 2) mean - 1 / (n - 2), n_obs defaulting to n_hap."""
        return adjust_l2(self.mean_r2, 1.0, self.n_hap if n_obs is None else int(n_obs))

    def rebin(self, edges) -> Tuple[np.ndarray, np.ndarray]:
        """Merge the fine bins into coarser ones: (sum_r2, counts) of the distances [edges[k], edges[k + 1]), one entry per
        consecutive pair of edges.  The edges are strictly increasing multiples of bin_width (an edge beyond the last bin
        stands for its end); anything else raises."""
        e = np.asarray(edges)
        if e.ndim != 1 or e.size < 2 or not np.issubdtype(e.dtype, np.integer):
            raise _lib.LdxError("rebin needs at least two integer edges")
        e = e.astype(np.int64)
        if (e < 0).any() or (np.diff(e) <= 0).any() or (e % self.bin_width != 0).any():
            raise _lib.LdxError(f"rebin edges must be increasing multiples of the bin width {self.bin_width}")
        idx = np.minimum(e // self.bin_width, self.n_bins)
        cs = np.concatenate([[0.0], np.cumsum(self.sum_r2)])
        cc = np.concatenate([[0], np.cumsum(self.counts)])
        return cs[idx[1:]] - cs[idx[:-1]], cc[idx[1:]] - cc[idx[:-1]]


def ld_decay(panel: PackedPanel, positions=None, window_bp: int = 250_000, window_snps: Optional[int] = None,
             bin_bp: int = 1000, keep=None, path: Optional[str] = None, workspace: Optional[torch.Tensor] = None,
             check_positions: bool = True, dosage: bool = False) -> LDDecay:
    """LD decay on the matrix-pipe band: per distance bin of width ``bin_bp``, the sum of r^2 and the number of pairs i > j
    with pos_i - pos_j <= window, both SNPs non-degenerate and -- with ``keep`` (bool [n]) -- both kept (include/ldx.h,
    ldx_ld_decay_dev).  r is the signed r of ld_triangle(fmt="r32"), bit for bit; the sums are exact integer sums of
    rint(2^32 r^2) and the bins exact, so the result is reproducible run to run and identical on both paths.

    ``window_snps`` counts the window, the distances and ``bin_bp`` in SNPs (positions 0 .. n-1).  At most DECAY_MAX_BINS
    bins: coarser curves come from ``LDDecay.rebin``.  ``path``: 'fp4' (default) or 'mfma'.  ``workspace``: a uint8 device
    tensor of ldx_ld_decay_workspace_bytes() bytes to reuse (one per launch that may be in flight).  The call is
    stream-ordered: the host reads nothing until ``.counts`` / ``.sum_r2`` are asked for.
    
    ``dosage`` is refused: this operator has no genotype-dosage form, and it never computes haplotype r in its place."""
    _dosage_refused("ld_decay", dosage)
    require_gpu()
    n = panel.n_snps
    pos, _, window = _band_positions(panel, positions, window_bp, window_snps, check_positions, "ld_decay")
    width = int(bin_bp)
    if width < 1:
        raise _lib.LdxError("bin_bp must be >= 1")
    n_bins = decay_bins(window, width)
    if n_bins > _lib.DECAY_MAX_BINS:
        least = min(window, DECAY_WINDOW_MAX) // _lib.DECAY_MAX_BINS + 1
        raise _lib.LdxError(f"{n_bins} bins > DECAY_MAX_BINS {_lib.DECAY_MAX_BINS}: the smallest admissible bin_bp for this "
                            f"window is {least}")
    keep_d = _keep_dev(keep, n, panel.device)
    pcode = _band_path(path)
    workspace = _band_workspace(lib.ldx_ld_decay_workspace_bytes, panel, workspace)
    sums = torch.empty(n_bins, dtype=torch.uint64, device=panel.device)
    counts = torch.empty(n_bins, dtype=torch.uint64, device=panel.device)
    _decay_launch(panel, pos, window, width, keep_d, pcode, sums, counts, workspace)
    res = LDDecay(sums, counts, width, window, panel.n_hap)
    res._keep = (pos, keep_d, workspace)   # alive until the launch is done
    return res


def _decay_launch(panel, pos, window, width, keep_d, pcode, sums, counts, workspace) -> None:
    check(lib.ldx_ld_decay_dev(*_phased_panel(panel), panel.n_snps, panel.n_hap, pos.data_ptr(), window, width, _ptr(keep_d),
                               pcode, sums.data_ptr(), counts.data_ptr(), sums.numel(), *_ws(workspace), _stream_ptr()),
          "ldx_ld_decay_dev")


# --------------------------------------------------------------------------- haplotype blocks (four-gamete test)
NOT_KEPT = 0xFFFFFFFF            # block_of of a SNP that is not kept (include/ldx.h, ldx_ld_blocks_dev)


def blocks_host(left, positions, window: int, keep=None) -> Tuple[np.ndarray, int, int]:
    """Host mirror of ldx_ld_blocks_dev, the scan only: (block_of uint32 [n], n_blocks, rm) from a ``left`` array
    (ldx_ld_fgt_dev's output).  With s the current block's first SNP, kept SNP i starts a new block iff there is no current
    block, or left[i] >= s + 1, or pos_i - pos_s > window; ``rm`` counts the starts the ``left`` rule caused (it outranks
    the window rule)."""
    left = np.asarray(left).astype(np.int64)
    pos = np.asarray(positions, dtype=np.int64)
    n = left.shape[0]
    if pos.shape != (n,):
        raise _lib.LdxError("positions must have one entry per SNP")
    kept = np.ones(n, dtype=bool) if keep is None else np.asarray(keep).astype(bool)
    block_of = np.full(n, NOT_KEPT, dtype=np.uint32)
    s, n_blocks, rm = -1, 0, 0
    for i in range(n):
        if not kept[i]:
            continue
        by_left = s >= 0 and left[i] >= s + 1
        if s < 0 or by_left or pos[i] - pos[s] > window:
            rm += int(by_left)
            s = i
            n_blocks += 1
        block_of[i] = n_blocks - 1
    return block_of, n_blocks, rm


@dataclass
class LDBlocks:
    """Haplotype blocks of one panel by the four-gamete test (ld_blocks).  ``left_dev`` / ``block_of_dev`` / ``n_out`` are
    the device tensors the two calls wrote (int32 views of the uint32 words); the host arrays are fetched when first asked
    for.  The partition is the greedy left-to-right one (Hudson & Kaplan), not Haploview's block-picking order."""

    left_dev: torch.Tensor
    block_of_dev: torch.Tensor
    n_out: torch.Tensor
    positions: object
    window: int
    min_count: int
    keep: Optional[np.ndarray] = None
    _host: Optional[tuple] = None

    def _fetch(self) -> tuple:
        if self._host is None:
            left = self.left_dev.cpu().numpy().view(np.uint32)
            block_of = self.block_of_dev.cpu().numpy().view(np.uint32)
            n_out = self.n_out.cpu().numpy().view(np.uint32)
            pos = self.positions.cpu().numpy() if isinstance(self.positions, torch.Tensor) else self.positions
            kept = np.flatnonzero(block_of != NOT_KEPT)
            b = block_of[kept].astype(np.int64)
            first = np.ones(kept.size, dtype=bool)
            first[1:] = b[1:] != b[:-1]
            last = np.ones(kept.size, dtype=bool)
            last[:-1] = first[1:]
            self._host = (left, block_of, int(n_out[0]), int(n_out[1]), kept[first], kept[last],
                          np.bincount(b, minlength=int(n_out[0])).astype(np.int64), np.asarray(pos, dtype=np.int64))
        return self._host

    @property
    def left(self) -> np.ndarray:
        """uint32 [n]: 1 + the nearest recombinant partner to the left, 0 if none."""
        return self._fetch()[0]

    @property
    def block_of(self) -> np.ndarray:
        """uint32 [n]: the 0-based block of every SNP, NOT_KEPT for a SNP that is not kept."""
        return self._fetch()[1]

    @property
    def n_blocks(self) -> int:
        return self._fetch()[2]

    @property
    def rm(self) -> int:
        """Block starts caused by a recombinant pair: Hudson & Kaplan's Rm restricted to the window."""
        return self._fetch()[3]

    @property
    def starts(self) -> np.ndarray:
        """int64 [n_blocks]: the first SNP of every block."""
        return self._fetch()[4]

    @property
    def ends(self) -> np.ndarray:
        """int64 [n_blocks]: the last kept SNP of every block (inclusive)."""
        return self._fetch()[5]

    @property
    def sizes(self) -> np.ndarray:
        """int64 [n_blocks]: kept SNPs per block."""
        return self._fetch()[6]

    @property
    def spans_bp(self) -> np.ndarray:
        """int64 [n_blocks]: pos[end] - pos[start] of every block (<= window)."""
        pos = self._fetch()[7]
        return pos[self.ends] - pos[self.starts]


def ld_blocks(panel: PackedPanel, positions=None, window_bp: int = 500_000, window_snps: Optional[int] = None,
              min_count: int = 1, min_freq: Optional[float] = None, keep=None, maf_min: float = 0.0,
              path: Optional[str] = None, workspace: Optional[torch.Tensor] = None,
              check_positions: bool = True, dosage: bool = False) -> LDBlocks:
    """Haplotype blocks by the four-gamete test on the matrix-pipe band (include/ldx.h, ldx_ld_fgt_dev + ldx_ld_blocks_dev).
    A pair i > j with pos_i - pos_j <= window, both SNPs kept, is recombinant when each of the four two-locus haplotypes
    occurs at least ``min_count`` times ("not ALT" is the other allele: missing codes count with REF); ``left[i]`` is 1 +
    the nearest recombinant partner to the left, and the blocks are the greedy left-to-right partition over it, cut by
    the window as well, so no block holds a recombinant pair.  Integer arithmetic throughout: identical on both paths.

    ``min_freq`` gives min_count = max(1, ceil(min_freq * n_hap)) (Haploview's rule: 0.01).  ``keep`` (bool [n]) and
    ``maf_min`` (keeps min(a, n - a) / n >= maf_min) combine into the keep mask; monomorphic SNPs are otherwise kept (they
    are compatible with everything).  ``window_snps`` counts the window in SNPs (positions 0 .. n-1).  ``path``: 'fp4'
    (default) or 'mfma'.  ``workspace``: a uint8 device tensor of ldx_ld_fgt_workspace_bytes() bytes to reuse.  The call is
    stream-ordered: the host reads nothing until a result property is asked for.
    
    ``dosage`` is refused: this operator has no genotype-dosage form, and it never computes haplotype r in its place."""
    _dosage_refused("ld_blocks", dosage)
    require_gpu()
    n = panel.n_snps
    pos, pos_h, window = _band_positions(panel, positions, window_bp, window_snps, check_positions, "ld_blocks")
    if min_freq is not None:
        if not 0.0 <= float(min_freq) <= 1.0:
            raise _lib.LdxError("min_freq must lie in [0, 1]")
        min_count = max(1, int(np.ceil(float(min_freq) * panel.n_hap)))
    min_count = int(min_count)
    if not 1 <= min_count <= panel.n_hap:
        raise _lib.LdxError(f"min_count must be 1 .. n_hap ({panel.n_hap}), got {min_count}")
    kept = _keep_mask(keep, n)
    if maf_min > 0.0:
        a = panel.alt_counts().astype(np.int64)
        common = np.minimum(a, panel.n_hap - a) >= float(maf_min) * panel.n_hap
        kept = common if kept is None else kept & common
    keep_d = None if kept is None else torch.from_numpy(kept.astype(np.uint8)).to(panel.device)
    pcode = _band_path(path)
    workspace = _band_workspace(lib.ldx_ld_fgt_workspace_bytes, panel, workspace)
    left = torch.empty(n, dtype=torch.int32, device=panel.device)
    block_of = torch.empty(n, dtype=torch.int32, device=panel.device)
    n_out = torch.empty(2, dtype=torch.int32, device=panel.device)
    _fgt_launch(panel, pos, window, min_count, keep_d, pcode, left, workspace)
    _blocks_launch(left, pos, keep_d, n, window, block_of, n_out)
    res = LDBlocks(left, block_of, n_out, pos if pos_h is None else pos_h, window, min_count, kept)
    res._keep = (pos, keep_d, workspace)   # alive until the launches are done
    return res


def _fgt_launch(panel, pos, window, min_count, keep_d, pcode, left, workspace) -> None:
    check(lib.ldx_ld_fgt_dev(panel.alt.data_ptr(), panel.acnt.data_ptr(), panel.n_snps, panel.n_hap, pos.data_ptr(), window,
                             min_count, _ptr(keep_d), pcode, left.data_ptr(), *_ws(workspace), _stream_ptr()), "ldx_ld_fgt_dev")


def _blocks_launch(left, pos, keep_d, n, window, block_of, n_out) -> None:
    check(lib.ldx_ld_blocks_dev(left.data_ptr(), pos.data_ptr(), _ptr(keep_d), n, window, block_of.data_ptr(),
                                n_out.data_ptr(), _stream_ptr()), "ldx_ld_blocks_dev")


# --------------------------------------------------------------------------- LD-independent regions
SPLIT_COST_SHIFT = 16            # cost[k] = cross[k] >> 16: units of 2^-16 r^2 (include/ldx.h, ldx_ld_split_dev)
SPLIT_SAT = (1 << 64) - 2        # sums of costs saturate here; a total that reaches it counts as wrapped
SPLIT_FLAGS = {1: "no cut set gives every region min_snps .. max_snps SNPs", 2: "the total cost reached 2^64 - 2"}
REGION_POS_MAX = 1 << 62         # region_positions refuses shifted positions from here on


def cross_host(r, positions, window: int, live=None) -> Tuple[np.ndarray, np.ndarray]:
    """Host mirror of ldx_ld_cross_dev over an r32 square (TriangleResult.r_matrix()): (sides uint64 [n, 2], cross uint64
    [n + 1]).  Pair i > j with pos_i - pos_j <= window (both SNPs ``live`` if given: a degenerate cell's term is 0 anyway)
    adds score_terms of its cell to sides[i][0] and sides[j][1]; cross is the prefix sum of right - left modulo 2^64."""
    r = np.asarray(r, dtype=np.float32)
    n = r.shape[0]
    pos = np.asarray(positions, dtype=np.int64)
    if pos.shape != (n,):
        raise _lib.LdxError("positions must have one entry per SNP")
    window = min(int(window), DECAY_WINDOW_MAX)
    rows, cols = np.tril_indices(n, -1)
    sel = pos[rows] - pos[cols] <= window
    if live is not None:
        ok = np.asarray(live, dtype=bool)
        sel &= ok[rows] & ok[cols]
    rows, cols = rows[sel], cols[sel]
    t = score_terms(r[rows, cols])
    sides = np.zeros((n, 2), dtype=np.uint64)
    np.add.at(sides[:, 0], rows, t)
    np.add.at(sides[:, 1], cols, t)
    cross = np.zeros(n + 1, dtype=np.uint64)
    cross[1:] = np.cumsum(sides[:, 1] - sides[:, 0], dtype=np.uint64)   # (uint64 arithmetic wraps: modulo 2^64)
    return sides, cross


def cross_pairs(positions, window: int, live) -> np.ndarray:
    """int64 [n + 1]: the pairs j < k <= i of ``live`` SNPs with pos_i - pos_j <= window, per cut k -- the number of terms
    behind cross[k].  From window_bounds: a prefix sum of (right partners - left partners)."""
    pos = np.asarray(positions, dtype=np.int64)
    n = pos.shape[0]
    lo, hi = window_bounds(pos, min(int(window), DECAY_WINDOW_MAX))
    ok = np.asarray(live, dtype=bool)
    pre = np.concatenate([[0], np.cumsum(ok.astype(np.int64))])
    k = np.arange(n)
    right = np.where(ok, pre[hi] - pre[k + 1], 0)
    left = np.where(ok, pre[k] - pre[lo], 0)
    return np.concatenate([[0], np.cumsum(right - left)]).astype(np.int64)


def split_feasible(n: int, min_snps: int, max_snps: int) -> bool:
    """Some m has m min_snps <= n <= m max_snps: n SNPs can be cut into regions of min_snps .. max_snps."""
    m = -(-n // max_snps)
    return m >= 1 and m * min_snps <= n


def split_host(cross, min_snps: int, max_snps: int) -> Tuple[np.ndarray, int]:
    """Host mirror of ldx_ld_split_dev's recurrence, a plain loop over the states: (cuts int64 ascending, total cost in
    units of 2^-16 r^2).  best[k] = min over p in [max(0, k - max_snps), k - min_snps] of best[p], plus cross[k] >> 16 for
    k < n; prev[k] the LARGEST p at the minimum; the cuts are the backtrack from n.  Raises LdxError when no cut set is
    admissible or the total reaches 2^64 - 2 (where the kernel's sums saturate)."""
    cross = np.asarray(cross, dtype=np.uint64)
    n = cross.shape[0] - 1
    min_snps, max_snps = int(min_snps), int(max_snps)
    if n < 1 or not 1 <= min_snps <= max_snps:
        raise _lib.LdxError("split_host needs n >= 1 and 1 <= min_snps <= max_snps")
    cost = (cross >> np.uint64(SPLIT_COST_SHIFT)).astype(np.float64)   # < 2^48: exact; +inf marks an infeasible state
    exact = [int(c) >> SPLIT_COST_SHIFT for c in cross.tolist()]
    best = np.full(n + 1, np.inf)
    total = [None] * (n + 1)        # the exact sums (Python integers) beside their float64 keys
    prev = np.full(n + 1, -1, dtype=np.int64)
    best[0], total[0] = 0.0, 0
    fits = True                      # every sum so far is below 2^53: the float64 keys order the states exactly
    for k in range(1, n + 1):
        a, b = max(0, k - max_snps), k - min_snps
        if b < 0:
            continue
        seg = best[a:b + 1]
        if fits:
            m = seg.min()
            if not np.isfinite(m):
                continue
            p = b - int(np.argmin(seg[::-1]))            # the largest p at the minimum
        else:
            cand = [q for q in range(a, b + 1) if total[q] is not None]
            if not cand:
                continue
            least = min(total[q] for q in cand)
            p = max(q for q in cand if total[q] == least)
        total[k] = total[p] + (exact[k] if k < n else 0)
        best[k] = float(total[k])
        prev[k] = p
        fits = fits and total[k] < (1 << 53)
    if total[n] is None:
        raise _lib.LdxError(f"no cut set gives every region {min_snps} .. {max_snps} SNPs (n = {n})")
    if total[n] >= SPLIT_SAT:
        raise _lib.LdxError("the total cost of the cuts reached 2^64 - 2")
    cuts = []
    k = int(prev[n])
    while k != 0:
        cuts.append(k)
        k = int(prev[k])
    return np.asarray(cuts[::-1], dtype=np.int64), int(total[n])


def region_positions(positions, region_of, window: Optional[int] = None) -> Tuple[np.ndarray, int]:
    """Positions under which a band call sees only pairs of one region: (positions', window') with positions'_i =
    positions_i + region_of_i (window + 1).  Distances inside a region are unchanged, any pair across a boundary is farther
    than ``window`` apart, and the result is still non-decreasing.  ``region_of``: one integer per SNP, non-decreasing,
    starting at 0.  ``window=None``: the largest region span (pos[last] - pos[first]), i.e. whole regions.  Raises LdxError
    if the shifted positions would reach 2^62."""
    pos = np.ascontiguousarray(np.asarray(positions, dtype=np.int64))
    reg = np.asarray(region_of)
    if reg.shape != pos.shape or pos.ndim != 1 or not (np.issubdtype(reg.dtype, np.integer) or reg.dtype == bool):
        raise _lib.LdxError("region_of must hold one integer per SNP")
    reg = reg.astype(np.int64)
    if pos.size == 0:
        raise _lib.LdxError("region_positions needs at least one SNP")
    if reg[0] != 0 or bool((np.diff(reg) < 0).any()):
        raise _lib.LdxError("region_of must be non-decreasing and start at 0")
    if pos.size > 1 and bool((np.diff(pos) < 0).any()):
        raise _lib.LdxError("positions must be non-decreasing (VCF order)")
    if window is None:
        first = np.concatenate([[True], reg[1:] != reg[:-1]])
        last = np.concatenate([first[1:], [True]])
        window = int((pos[last] - pos[first]).max())
    window = int(window)
    if window < 0:
        raise _lib.LdxError("the window must be >= 0")
    if int(pos[-1]) + int(reg[-1]) * (window + 1) >= REGION_POS_MAX or int(pos[0]) <= -REGION_POS_MAX:
        raise _lib.LdxError("region_positions: the shifted positions would reach 2^62")
    return pos + reg * np.int64(window + 1), window


@dataclass
class LDCross:
    """One-sided LD scores and the cross-LD profile of one panel (ld_cross).  ``sides`` (uint64 [n, 2]: left, right) and
    ``cross`` (uint64 [n + 1]) are the device tensors the call wrote, in units of 2^-32 r^2; the host arrays are fetched
    when first asked for."""

    sides: torch.Tensor
    cross: torch.Tensor
    positions: object
    window: int
    n_hap: int
    panel: Optional[PackedPanel] = None
    _host: Optional[tuple] = None
    _pairs: Optional[np.ndarray] = None

    def _fetch(self) -> tuple:
        if self._host is None:
            s = self.sides.cpu().numpy().astype(np.float64) / SCORE_SCALE
            self._host = (s[:, 0].copy(), s[:, 1].copy(), self.cross.cpu().numpy().astype(np.float64) / SCORE_SCALE)
        return self._host

    @property
    def left(self) -> np.ndarray:
        """float64 [n]: the sum of r^2 over every SNP's in-window partners to its left (a one-sided LD score, self excluded)."""
        return self._fetch()[0]

    @property
    def right(self) -> np.ndarray:
        """float64 [n]: the same over the partners to its right."""
        return self._fetch()[1]

    @property
    def cross_r2(self) -> np.ndarray:
        """float64 [n + 1]: the sum of r^2 over the in-window pairs j < k <= i, per cut k."""
        return self._fetch()[2]

    @property
    def live(self) -> np.ndarray:
        return (self.panel.alt_counts().astype(np.int64) * self.panel.ref_counts().astype(np.int64)) > 0

    @property
    def pairs(self) -> np.ndarray:
        """int64 [n + 1]: the in-window pairs of non-degenerate SNPs that straddle each cut (cross_pairs)."""
        if self._pairs is None:
            pos = self.positions.cpu().numpy() if isinstance(self.positions, torch.Tensor) else self.positions
            self._pairs = cross_pairs(pos, self.window, self.live)
        return self._pairs

    @property
    def mean_r2(self) -> np.ndarray:
        """float64 [n + 1]: cross_r2 / pairs, NaN where no pair straddles the cut."""
        c = self.pairs
        return np.where(c > 0, self.cross_r2 / np.maximum(c, 1), np.nan)


def _cross_launch(panel, pos, window, pcode, sides, cross, workspace) -> None:
    check(lib.ldx_ld_cross_dev(*_phased_panel(panel), panel.n_snps, panel.n_hap, pos.data_ptr(), window, pcode,
                               sides.data_ptr(), cross.data_ptr(), *_ws(workspace), _stream_ptr()), "ldx_ld_cross_dev")


def _split_launch(cross, n, min_snps, max_snps, cuts, n_out, workspace) -> None:
    check(lib.ldx_ld_split_dev(cross.data_ptr(), n, min_snps, max_snps, cuts.data_ptr(), n_out.data_ptr(),
                               *_ws(workspace), _stream_ptr()), "ldx_ld_split_dev")


def ld_cross(panel: PackedPanel, positions=None, window_bp: int = 1_000_000, window_snps: Optional[int] = None,
             path: Optional[str] = None, workspace: Optional[torch.Tensor] = None, check_positions: bool = True,
             dosage: bool = False) -> LDCross:
    """The cross-LD profile on the matrix-pipe band (include/ldx.h, ldx_ld_cross_dev): ld_score's sweep with every SNP's
    score kept in two halves -- the r^2 of its in-window partners to the left and to the right -- and their prefix sum
    cross[k], the r^2 summed over the in-window pairs j < k <= i: the LD a region boundary before SNP k would cut.  r is
    the signed r of ld_triangle(fmt="r32"), bit for bit; the sums are exact integer sums of rint(2^32 r^2): reproducible
    run to run and identical on both paths.

    Positions, window, ``path`` and ``workspace`` (ldx_ld_cross_workspace_bytes() bytes) as for ld_score.  The call is
    stream-ordered: the host reads nothing until a result property is asked for.
    ``dosage`` is refused: this operator has no genotype-dosage form, and it never computes haplotype r in its place."""
    _dosage_refused("ld_cross", dosage)
    require_gpu()
    n = panel.n_snps
    pos, pos_h, window = _band_positions(panel, positions, window_bp, window_snps, check_positions, "ld_cross")
    pcode = _band_path(path)
    workspace = _band_workspace(lib.ldx_ld_cross_workspace_bytes, panel, workspace)
    sides = torch.empty((n, 2), dtype=torch.uint64, device=panel.device)
    cross = torch.empty(n + 1, dtype=torch.uint64, device=panel.device)
    _cross_launch(panel, pos, window, pcode, sides, cross, workspace)
    res = LDCross(sides, cross, pos if pos_h is None else pos_h, window, panel.n_hap, panel)
    res._keep = (pos, workspace)   # alive until the launch is done
    return res


@dataclass
class LDRegions:
    """Approximately LD-independent regions of one panel (ld_regions): the cuts of minimum total cross-LD with every region
    min_snps .. max_snps SNPs long.  ``cuts`` (int64, ascending): a cut c is a boundary before SNP c."""

    cuts: np.ndarray
    n_snps: int
    positions: np.ndarray
    window: int
    min_snps: int
    max_snps: int
    cross: Optional[LDCross] = None
    cuts_dev: Optional[torch.Tensor] = None

    @property
    def n_regions(self) -> int:
        return int(self.cuts.size) + 1

    @property
    def starts(self) -> np.ndarray:
        """int64 [n_regions]: the first SNP of every region."""
        return np.concatenate([[0], self.cuts]).astype(np.int64)

    @property
    def ends(self) -> np.ndarray:
        """int64 [n_regions]: the last SNP of every region (inclusive)."""
        return np.concatenate([self.cuts - 1, [self.n_snps - 1]]).astype(np.int64)

    @property
    def sizes(self) -> np.ndarray:
        return self.ends - self.starts + 1

    @property
    def region_of(self) -> np.ndarray:
        """int64 [n]: the 0-based region of every SNP."""
        return np.repeat(np.arange(self.n_regions, dtype=np.int64), self.sizes)

    @property
    def spans_bp(self) -> np.ndarray:
        """int64 [n_regions]: pos[end] - pos[start] of every region."""
        return self.positions[self.ends] - self.positions[self.starts]

    @property
    def cross_at_cuts(self) -> np.ndarray:
        """float64 [n_regions - 1]: the r^2 that crosses each cut (LDCross.cross_r2 at the cuts)."""
        return self.cross.cross_r2[self.cuts]

    @property
    def total_cross(self) -> float:
        return float(self.cross_at_cuts.sum())


def ld_regions(panel: PackedPanel, positions=None, window_bp: int = 1_000_000, window_snps: Optional[int] = None,
               min_snps: int = 100, max_snps: int = 10_000, path: Optional[str] = None) -> LDRegions:
    """Split a panel into approximately LD-independent regions (include/ldx.h, ldx_ld_cross_dev + ldx_ld_split_dev): the cut
    set that minimises the sum over its cuts of the in-window r^2 crossing each one, every region holding min_snps ..
    max_snps SNPs -- the objective of ldetect (Berisa & Pickrell 2016) and bigsnpr's snp_ldsplit with additive cuts.  Costs
    are compared as integers (cross >> 16, units of 2^-16 r^2) and ties go to the later cut, so the result is reproducible
    and equal to split_host over the profile.  Both kernels run back to back on the stream; the cuts are read at the end.

    Raises LdxError before any launch when no m has m min_snps <= n <= m max_snps, naming the nearest admissible
    max_snps."""
    require_gpu()
    n = panel.n_snps
    min_snps, max_snps = int(min_snps), int(max_snps)
    if not 1 <= min_snps <= max_snps:
        raise _lib.LdxError(f"need 1 <= min_snps <= max_snps (got {min_snps}, {max_snps})")
    if not split_feasible(n, min_snps, max_snps):
        if n < min_snps:
            raise _lib.LdxError(f"{n} SNPs cannot form a region of min_snps = {min_snps}: no max_snps is admissible")
        raise _lib.LdxError(f"{n} SNPs cannot be cut into regions of {min_snps} .. {max_snps} SNPs: the nearest admissible "
                            f"max_snps is {-(-n // (n // min_snps))}")
    cr = ld_cross(panel, positions, window_bp, window_snps, path)
    cuts = torch.empty(max(1, n // min_snps), dtype=torch.int32, device=panel.device)
    n_out = torch.empty(2, dtype=torch.int32, device=panel.device)
    ws = torch.empty(lib.ldx_ld_split_workspace_bytes(n), dtype=torch.uint8, device=panel.device)
    _split_launch(cr.cross, n, min_snps, min(max_snps, 0xFFFFFFFF), cuts, n_out, ws)
    count, flag = (int(v) for v in n_out.cpu().numpy().view(np.uint32))
    if flag:
        raise _lib.LdxError(f"ldx_ld_split_dev: {SPLIT_FLAGS.get(flag, flag)}")
    pos = cr.positions.cpu().numpy() if isinstance(cr.positions, torch.Tensor) else cr.positions
    return LDRegions(cuts[:count].cpu().numpy().view(np.uint32).astype(np.int64), n, np.asarray(pos, dtype=np.int64),
                     cr.window, min_snps, max_snps, cr, cuts)


def _region_band(panel: PackedPanel, positions, window_bp, window_snps, regions, check_positions: bool, what: str):
    """_band_positions, through region_positions when ``regions`` (an LDRegions or a region_of array) is given: the band then
    sees the pairs inside a region only.  ``window_bp=None`` (whole regions) needs ``regions``.  With ``regions`` the
    positions are read on the host."""
    if regions is None:
        if window_bp is None and window_snps is None:
            raise _lib.LdxError(f"{what}: window_bp=None (whole regions) needs regions=")
        return _band_positions(panel, positions, window_bp, window_snps, check_positions, what)
    n = panel.n_snps
    region_of = regions.region_of if isinstance(regions, LDRegions) else \
        (regions.cpu().numpy() if isinstance(regions, torch.Tensor) else np.asarray(regions))
    if window_snps is not None:
        pos_h, window = np.arange(n, dtype=np.int64), int(window_snps)
    else:
        if positions is None:
            raise _lib.LdxError(f"{what} needs positions (or window_snps)")
        pos_h = positions.cpu().numpy() if isinstance(positions, torch.Tensor) else np.asarray(positions)
        window = None if window_bp is None else int(window_bp)
    if pos_h.shape != (n,):
        raise _lib.LdxError("positions must have one entry per SNP")
    if window is not None and window < 0:
        raise _lib.LdxError("the window must be >= 0")
    shifted, window = region_positions(pos_h, region_of, window)
    return _band_positions(panel, shifted, window, None, check_positions, what)


# --------------------------------------------------------------------------- R x without the matrix, ridge solves
PROD_SCALE_BITS = 40             # sums are integers in units of 2^-40 (include/ldx.h, ldx_ld_matvec_dev)
PROD_CLAMP = float(1 << 22)      # |v x| beyond it is clamped before scaling (keeps the int64 conversion defined)
MAX_RHS = 8
RIDGE_BATCH = 8                  # CG iterations enqueued between two reads of the convergence flags


def prod_terms(v, x) -> np.ndarray:
    """Host mirror of the kernel's term (include/ldx.h, ldx_ld_matvec_dev): rint(2^40 * clamp(v x, -+2^22)) as int64, from
    float32 values v (r cells for power 1; ``prod_values(r, 2)`` for power 2) and float32 weights x, broadcast against each
    other.  The fp64 product of two float32 is exact, so is the scaling: one round-half-even."""
    v = np.asarray(v, dtype=np.float32).astype(np.float64)
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    p = np.clip(v * x, -PROD_CLAMP, PROD_CLAMP)
    return np.rint(np.ldexp(p, PROD_SCALE_BITS)).astype(np.int64)


def prod_values(r, power: int = 1) -> np.ndarray:
    """The value the terms multiply: the float32 r cell (power 1) or r *f32 r, ONE float32 multiply (power 2: what
    score_terms scales)."""
    r = np.asarray(r, dtype=np.float32)
    if power == 1:
        return r
    if power == 2:
        return np.multiply(r, r, dtype=np.float32)
    raise _lib.LdxError(f"power must be 1 or 2 (got {power!r})")


def _pow2(e: torch.Tensor) -> torch.Tensor:
    """2^e as float64 for an int64 tensor e in [-1022, 1023], built from the exponent bits: exact on every device."""
    return ((e + 1023) << 52).view(torch.float64)


def matvec_rhs(x, n_snps: int, power: int = 1, check_finite: bool = True, device=None):
    """Validate and scale the right-hand sides of ld_matvec.  ``x``: [n] or [n, k] (1 <= k <= 8), numpy or torch, real.
    Each column is multiplied by 2^-e, e the smallest integer with max |x| 2^-e <= 1 (the scaled maximum lies in (0.5, 1];
    a column within (0.5, 1] already, a 0/1 annotation say, and an all-zero column keep e = 0) -- exact -- and only then
    converted to float32.  Returns (x32 float32 [n, k] contiguous,
    e int64 [k], squeeze: x was one-dimensional), tensors on ``device`` (default: where x is)."""
    if power not in (1, 2):
        raise _lib.LdxError(f"power must be 1 or 2 (got {power!r})")
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if t.is_complex() or t.dtype == torch.bool:
        raise _lib.LdxError(f"x must be real (got {t.dtype})")
    squeeze = t.ndim == 1
    if squeeze:
        t = t[:, None]
    if t.ndim != 2 or t.shape[0] != n_snps:
        raise _lib.LdxError(f"x must have shape [n_snps] or [n_snps, k] (n_snps = {n_snps}), got {tuple(x.shape)}")
    if not 1 <= t.shape[1] <= MAX_RHS:
        raise _lib.LdxError(f"1 to {MAX_RHS} right-hand sides per call (got {t.shape[1]})")
    if device is not None:
        t = t.to(device)
    t = t.to(torch.float64)
    if check_finite and not bool(torch.isfinite(t).all().item()):
        raise _lib.LdxError("x must be finite")
    big = t.abs().amax(dim=0)
    mant, e = torch.frexp(big)                              # big = mant 2^e, mant in [0.5, 1)
    e = e.to(torch.int64) - (mant == 0.5).to(torch.int64)   # the smallest e with big 2^-e <= 1 (a power of two: exactly 1)
    e = torch.where(big > 0, e, torch.zeros_like(e)).clamp(-1000, 1000)
    x32 = (t * _pow2(-e)).to(torch.float32).contiguous()
    return x32, e, squeeze


@dataclass
class LDProduct:
    """A banded LD matrix-vector product (ld_matvec).  ``sums``: the device int64 tensor [n, k] the kernel wrote, in units
    of 2^(e_k - 40); ``exps``: device int64 [k], the columns' exponents e; ``x32``: the float32 values actually multiplied
    (x 2^-e, rounded to float32 once)."""

    sums: torch.Tensor
    exps: torch.Tensor
    x32: torch.Tensor
    window: int
    power: int
    squeeze: bool = False

    def values(self) -> torch.Tensor:
        """float64 device tensor [n, k] ([n] for a one-dimensional x): sums 2^(e - 40), i.e. R_w x (power 2: (R_w o R_w) x)."""
        y = self.sums.to(torch.float64) * _pow2(self.exps - PROD_SCALE_BITS)
        return y[:, 0] if self.squeeze else y

    def x(self) -> torch.Tensor:
        """float64 device tensor: the vectors the product is exactly that of (x32 rescaled), shaped like ``values()``."""
        y = self.x32.to(torch.float64) * _pow2(self.exps)
        return y[:, 0] if self.squeeze else y


def _matvec_launch(panel: PackedPanel, pos: torch.Tensor, window: int, x32: torch.Tensor, power: int, pcode: int,
                   workspace: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    n, k = x32.shape
    workspace = _band_workspace(lib.ldx_ld_matvec_workspace_bytes, panel, workspace)
    sums = torch.empty((n, k), dtype=torch.int64, device=panel.device)
    check(lib.ldx_ld_matvec_dev(*_phased_panel(panel), n, panel.n_hap, pos.data_ptr(), window, x32.data_ptr(), k, power, pcode,
                                sums.data_ptr(), *_ws(workspace), _stream_ptr()), "ldx_ld_matvec_dev")
    return sums, workspace


def ld_matvec(panel: PackedPanel, x, positions=None, window_bp: int = 1_000_000, window_snps: Optional[int] = None,
              power: int = 1, path: str = "auto", workspace: Optional[torch.Tensor] = None, check_positions: bool = True,
              check_finite: bool = True, regions=None, dosage: bool = False) -> LDProduct:
    """y = R_w x on the matrix-pipe band, without the matrix (include/ldx.h, ldx_ld_matvec_dev): for every SNP i the sum of
    r_ij x_j over the SNPs j with |pos_i - pos_j| <= window (i included, r_ii = r_matrix()'s diagonal), r the signed r of
    ld_triangle(fmt="r32") bit for bit; ``power=2`` sums r^2 x_j instead (r^2 one float32 multiply) -- the LD score of a
    continuous annotation x.  ``x``: [n] or [n, k], k <= 8 right-hand sides in one band sweep; numpy or a device tensor,
    float32 or float64.  Each column is scaled by a power of two to max |x| <= 1 and converted to float32 (matvec_rhs); the
    kernel adds rint(2^40 r x) as 64-bit integers, so the result is reproducible run to run and identical on both paths,
    every term within 2^-41 (times the column's scale) of exact.

    Positions and window as for ld_score.  ``path``: 'auto' / 'fp4' (the FP4 band) or 'mfma' (the int8 band: identical
    sums).  ``workspace``: a uint8 device tensor of ldx_ld_matvec_workspace_bytes() bytes to reuse (one per launch that may
    be in flight).  The call is stream-ordered; with ``check_positions`` and ``check_finite`` off and device tensors in it
    reads nothing on the host.  ``LDProduct.values()`` is the float64 result on the device.

    ``regions`` (an LDRegions or a region_of array; default None: no change) restricts the product to the block-diagonal
    R_B x: r_ij counts only for i and j of one region (region_positions; the positions are then read on the host), and
    ``window_bp=None`` means whole regions.
    ``dosage`` is refused: this operator has no genotype-dosage form, and it never computes haplotype r in its place."""
    _dosage_refused("ld_matvec", dosage)
    require_gpu()
    pos, _, window = _region_band(panel, positions, window_bp, window_snps, regions, check_positions, "ld_matvec")
    x32, e, squeeze = matvec_rhs(x, panel.n_snps, power, check_finite, panel.device)
    sums, workspace = _matvec_launch(panel, pos, window, x32, power, PATHS[path], workspace)
    res = LDProduct(sums, e, x32, window, power, squeeze)
    res._keep = (pos, workspace)   # alive until the launch is done
    return res


@dataclass
class RidgeResult:
    """ld_ridge's solution.  ``beta``: float64 device tensor shaped like z (NaN in a column reported ``indefinite``);
    per column (numpy): ``iterations`` taken, ``converged`` (||r|| <= tol ||z|| on the recurrence residual),
    ``indefinite`` (a direction with p.Ap <= 0 was met: the windowed matrix is not positive definite; no solution is
    returned) and ``residual`` = ||r|| / ||z|| of the recurrence when the column stopped."""

    beta: torch.Tensor
    iterations: np.ndarray
    converged: np.ndarray
    indefinite: np.ndarray
    residual: np.ndarray


def cg_solve(product, z: torch.Tensor, lam: float, tol: float = 1e-6, max_iter: int = 1000,
             batch: int = RIDGE_BATCH) -> RidgeResult:
    """Conjugate gradients for (R + lam I) beta = z, the columns of ``z`` (float64 [n, k]) side by side with per-column
    step sizes.  ``product(P)`` returns (R Q, Q) for a float64 [n, k] tensor P, Q being the vectors it really multiplied
    (P rounded to what the product can represent; Q = P for an exact product): the recurrence then steps along Q, so beta
    and the residual stay consistent with the products that were computed.  Step and update coefficients are the local
    ones (alpha = p.r / p.Ap, the next direction A-orthogonalised against p), which hold for a rounded direction too.  A
    column stops when ||r|| <= tol ||z|| or when p.Ap <= 0 (``indefinite``); a stopped column keeps its beta and multiplies
    zeros from then on.  The flags are read on the host once per ``batch`` iterations."""
    if z.ndim != 2:
        raise _lib.LdxError("cg_solve: z must be [n, k]")
    z = z.to(torch.float64)
    k = z.shape[1]
    lam = float(lam)
    beta = torch.zeros_like(z)
    r = z.clone()
    z2 = (z * z).sum(dim=0)
    bound = (float(tol) ** 2) * z2
    rs = z2.clone()
    converged = rs <= bound                       # an all-zero column: beta = 0
    active = ~converged
    indefinite = torch.zeros(k, dtype=torch.bool, device=z.device)
    iters = torch.zeros(k, dtype=torch.int64, device=z.device)
    zero = torch.zeros((), dtype=torch.float64, device=z.device)
    p = torch.where(active, r, zero)
    for it in range(int(max_iter)):
        rq, p = product(p)
        ap = rq + lam * p
        pap = (p * ap).sum(dim=0)
        bad = active & ~(pap > 0)                 # (a NaN counts as not positive)
        indefinite |= bad
        active = active & ~bad
        alpha = torch.where(active, (p * r).sum(dim=0) / pap, zero)
        beta = beta + alpha * p
        r = r - alpha * ap
        rs = torch.where(active, (r * r).sum(dim=0), rs)
        iters += active
        done = active & (rs <= bound)
        converged |= done
        active = active & ~done
        gamma = torch.where(active, -(r * ap).sum(dim=0) / pap, zero)
        p = torch.where(active, r + gamma * p, zero)
        if (it + 1) % int(batch) == 0 and not bool(active.any().item()):
            break
    beta = torch.where(indefinite, torch.full_like(zero, float("nan")), beta)
    z2h = z2.cpu().numpy()
    res = np.sqrt(rs.cpu().numpy() / np.where(z2h > 0, z2h, 1.0))
    return RidgeResult(beta, iters.cpu().numpy(), converged.cpu().numpy(), indefinite.cpu().numpy(), res)


def ld_ridge(panel: PackedPanel, z, positions=None, window_bp: int = 1_000_000, window_snps: Optional[int] = None,
             lam: float = 1.0, tol: float = 1e-6, max_iter: int = 1000, path: str = "auto",
             check_positions: bool = True, regions=None, band: Optional["LDBand"] = None) -> RidgeResult:
    """Solve (R_w + lam I) beta = z by conjugate gradients on ld_matvec -- ridge / infinitesimal polygenic scores from
    summary statistics, R_w never formed.  ``z``: [n] or [n, k], k <= 8 columns solved side by side (one ld_matvec launch per
    iteration for all of them).  Before each product the search direction is replaced by the float32 vector the kernel
    really multiplies (LDProduct.x()), so the only product error left is the kernel's 2^-41 term rounding.  A windowed R
    need not be positive definite: a column that meets p.Ap <= 0 is reported ``indefinite`` with NaN in beta (cg_solve).

    ``regions`` (an LDRegions or a region_of array; default None: no change) solves with the block-diagonal R_B instead
    (ld_matvec's ``regions``).  With whole-region windows (``window_bp=None``) and no missing codes every block is the
    correlation matrix of its SNPs' ALT indicators, up to the float32 rounding of the cells -- positive semidefinite --, so
    ``indefinite`` cannot then come from window truncation.

    ``band`` (an LDBand of this panel from ld_band; default None: no change): every product is read from the stored band
    (LDBand.matvec: a sweep over the stored cells, the same int64 sums as ld_matvec on the band's window, hence the same iterates)
    instead of re-deriving every r cell on the matrix cores; positions and window are then the band's, and ``positions``,
    the window arguments, ``path`` and ``regions`` are not read.  A pairwise-complete haplotype band
    (ld_band(missing="pairwise")) is taken as it is -- the layout and the terms are the same -- and is the route to a ridge solve
    on a panel with missing calls; its matrix is estimated pair by pair over different observations, so it need not be
    positive semidefinite even on whole regions, and ``indefinite`` can be reported."""
    if band is not None:
        if band.dosage:
            raise _lib.LdxError("ld_ridge: band= needs a haplotype band (ld_matvec has no genotype-dosage form)")
        if band.n_snps != panel.n_snps:
            raise _lib.LdxError(f"ld_ridge: band= holds {band.n_snps} SNPs, the panel {panel.n_snps}")
    dev = require_gpu()
    if band is not None:
        pos, window = None, band.window
    else:
        pos, _, window = _region_band(panel, positions, window_bp, window_snps, regions, check_positions, "ld_ridge")
    zt = z if isinstance(z, torch.Tensor) else torch.as_tensor(np.asarray(z))
    squeeze = zt.ndim == 1
    matvec_rhs(zt, panel.n_snps)   # shape, column count, finiteness
    zt = (zt[:, None] if squeeze else zt).to(panel.device, dtype=torch.float64)
    if not (float(lam) >= 0.0 and np.isfinite(float(lam))):
        raise _lib.LdxError(f"lam must be a finite number >= 0 (got {lam})")
    ws = None if band is not None else \
        torch.empty(lib.ldx_ld_matvec_workspace_bytes(panel.n_snps, panel.n_hap), dtype=torch.uint8, device=panel.device)
    pcode = PATHS[path]

    def product(p):
        x32, e, _ = matvec_rhs(p, panel.n_snps, 1, False)
        if band is not None:
            sums = band._matvec_launch(x32, 1)
        else:
            sums, _ = _matvec_launch(panel, pos, window, x32, 1, pcode, ws)
        lp = LDProduct(sums, e, x32, window, 1)
        return lp.values(), lp.x()

    res = cg_solve(product, zt, lam, tol, max_iter)
    if squeeze:
        res.beta = res.beta[:, 0]
    del dev
    return res


# --------------------------------------------------------------------------- stored bands
CROSS_SCALE = SCORE_SCALE        # cross-score sums are integers in units of 2^-32 r1 r2 (include/ldx.h, ldx_band_score_dev)
BAND_WINDOW_MAX = 1 << 52        # larger windows act as 2^52 (include/ldx.h, "stored bands")


def band_layout_host(positions, window: int) -> Tuple[np.ndarray, np.ndarray]:
    """Host mirror of ldx_ld_band_layout_dev (include/ldx.h): ``(lo uint32 [n], offsets uint64 [n + 1])`` of the lower band of
    ``window`` over non-decreasing positions -- lo[i] the first j <= i with pos_i - pos_j <= window, offsets the prefix sum
    of i - lo[i]; cell (i, j), lo[i] <= j < i, is word offsets[i] + j - lo[i]."""
    pos = np.asarray(positions, dtype=np.int64)
    window = min(int(window), BAND_WINDOW_MAX)
    if window < 0:
        raise _lib.LdxError("the window must be >= 0")
    if pos.ndim != 1 or pos.size < 1:
        raise _lib.LdxError("positions must be a non-empty vector")
    if pos.size > 1 and bool((pos[1:] < pos[:-1]).any()):
        raise _lib.LdxError("positions must be non-decreasing (VCF order)")
    lo, _ = window_bounds(pos, window)
    offsets = np.zeros(pos.size + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(np.arange(pos.size, dtype=np.int64) - lo).astype(np.uint64)
    return lo.astype(np.uint32), offsets


def cross_terms(a, b) -> np.ndarray:
    """Host mirror of the cross-score term (include/ldx.h, ldx_band_score_dev): T(a, b) = rint(2^32 * (a *f32 b)) as int64,
    from float32 cells.  One float32 multiply, then exact scaling and round-half-even; T(c, c) is score_terms(c)."""
    p = np.multiply(np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32), dtype=np.float32)
    return np.rint(np.ldexp(p.astype(np.float64), 32)).astype(np.int64)


def _same_layout(a: "LDBand", b: "LDBand") -> bool:
    """Two bands share a layout: same SNP count, window and positions (compared where they live)."""
    if a.n_snps != b.n_snps or a.window != b.window or a.n_cells != b.n_cells:
        return False
    pa, pb = a.positions, b.positions
    if pa is pb:
        return True
    if isinstance(pa, torch.Tensor) and isinstance(pb, torch.Tensor):
        return bool(torch.equal(pa, pb.to(pa.device)))
    ha = pa.cpu().numpy() if isinstance(pa, torch.Tensor) else np.asarray(pa)
    hb = pb.cpu().numpy() if isinstance(pb, torch.Tensor) else np.asarray(pb)
    return bool(np.array_equal(ha, hb))


@dataclass
class LDBand:
    """The windowed LD matrix of one panel, stored (ld_band; include/ldx.h, "stored bands").  ``values``: float32 device
    tensor [n_cells], the signed r of every pair i > j with pos_i - pos_j <= window, once each -- ld_triangle(fmt="r32")'s
    cells bit for bit (its ``dosage=True`` cells for a dosage band); ``lo`` (int32 bit pattern of uint32 [n]) and
    ``offsets`` (int64 bit pattern of uint64 [n + 1]): cell (i, j), lo[i] <= j < i, is ``values[offsets[i] + j - lo[i]]``;
    ``diag``: float32 [n], r_matrix()'s diagonal (not part of ``values``).  ``positions``: what ld_band was given (numpy, or
    the device tensor); ``window``: the window in their units.  A pairwise-complete band (``missing == "pairwise"``) has the
    same layout with ld_rect(missing="pairwise")'s cells and a +1 / -0.0 diagonal, so ``to_csr``, ``to_dense``, ``matvec``,
    ld_ridge(band=) and ld_cross_score work on it as they are."""

    values: torch.Tensor
    lo: torch.Tensor
    offsets: torch.Tensor
    diag: torch.Tensor
    positions: object
    window: int
    dosage: bool = False
    n_hap: int = 0
    _host: Optional[tuple] = None
    missing: Optional[str] = None   # "pairwise": the cells are ld_rect(missing="pairwise")'s (ld_band(missing="pairwise"))
    em: bool = False                # the cells are ld_em's r or D' (ld_em_band): ``missing`` is then ld_em's

    @property
    def n_snps(self) -> int:
        return int(self.lo.numel())

    @property
    def n_cells(self) -> int:
        return int(self.values.numel())

    def layout(self) -> Tuple[np.ndarray, np.ndarray]:
        """``(lo, offsets)`` as int64 numpy arrays, fetched once."""
        if self._host is None:
            self._host = (self.lo.cpu().numpy().view(np.uint32).astype(np.int64),
                          self.offsets.cpu().numpy().view(np.uint64).astype(np.int64))
        return self._host

    def row(self, i: int) -> Tuple[np.ndarray, np.ndarray]:
        """``(columns, r)`` of row i's stored cells: the SNPs j < i inside the window, ascending, and their float32 r."""
        lo, off = self.layout()
        i = int(i)
        if not 0 <= i < self.n_snps:
            raise _lib.LdxError(f"row {i} outside 0..{self.n_snps - 1}")
        return np.arange(lo[i], i, dtype=np.int64), self.values[int(off[i]): int(off[i + 1])].cpu().numpy()

    def to_csr(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The symmetric windowed matrix as ``(indptr int64 [n + 1], indices int64, data float32)`` numpy arrays, rows
        sorted by column: both orientations of every stored pair and the diagonal (scipy.sparse.csr_matrix takes the
        triple as it is; nothing here needs scipy)."""
        lo, off = self.layout()
        n = self.n_snps
        vals = self.values.cpu().numpy()
        diag = self.diag.cpu().numpy()
        length = np.arange(n, dtype=np.int64) - lo
        rows_l = np.repeat(np.arange(n, dtype=np.int64), length)                 # the stored cells' (i, j)
        cols_l = np.arange(off[n], dtype=np.int64) - np.repeat(off[:-1] - lo, length)
        ii = np.concatenate([rows_l, np.arange(n, dtype=np.int64), cols_l])
        jj = np.concatenate([cols_l, np.arange(n, dtype=np.int64), rows_l])
        dd = np.concatenate([vals, diag, vals])
        order = np.lexsort((jj, ii))
        indptr = np.zeros(n + 1, dtype=np.int64)
        indptr[1:] = np.cumsum(np.bincount(ii, minlength=n))
        return indptr, jj[order], dd[order].astype(np.float32)

    def to_dense(self, rows: Optional[Tuple[int, int]] = None) -> np.ndarray:
        """float32 [r1 - r0, r1 - r0] numpy square of the rows / columns ``rows`` = (r0, r1) (default: all -- for small
        checks): the stored cells in both orientations, the diagonal, and +0.0 outside the window."""
        lo, off = self.layout()
        r0, r1 = (0, self.n_snps) if rows is None else (int(rows[0]), int(rows[1]))
        if not 0 <= r0 <= r1 <= self.n_snps:
            raise _lib.LdxError(f"rows {rows} outside 0..{self.n_snps}")
        out = np.zeros((r1 - r0, r1 - r0), dtype=np.float32)
        if r1 == r0:
            return out
        vals = self.values[int(off[r0]): int(off[r1])].cpu().numpy()
        diag = self.diag[r0:r1].cpu().numpy()
        for i in range(r0, r1):
            j0 = max(int(lo[i]), r0)
            seg = vals[int(off[i] - off[r0]) + (j0 - int(lo[i])): int(off[i + 1] - off[r0])]
            out[i - r0, j0 - r0: i - r0] = seg
            out[j0 - r0: i - r0, i - r0] = seg
            out[i - r0, i - r0] = diag[i - r0]
        return out

    def _matvec_launch(self, x32: torch.Tensor, power: int) -> torch.Tensor:
        n, k = x32.shape
        sums = torch.empty((n, k), dtype=torch.int64, device=self.values.device)
        check(lib.ldx_band_matvec_dev(_ptr(self.values) if self.n_cells else None, self.diag.data_ptr(), self.lo.data_ptr(),
                                      self.offsets.data_ptr(), n, x32.data_ptr(), k, power, sums.data_ptr(), _stream_ptr()),
              "ldx_band_matvec_dev")
        return sums

    def matvec(self, x, power: int = 1, check_finite: bool = True) -> LDProduct:
        """ld_matvec from the stored band (include/ldx.h, ldx_band_matvec_dev): the same right-hand-side scaling, terms and
        int64 sums -- bit for bit ld_matvec's on the band's window for a haplotype band -- as one sweep over ``values``
        instead of a pass over the panel on the matrix cores (about three times faster than ld_matvec with
        one right-hand side; with eight it is currently slower, so keep ld_matvec for wide batches).  On a
        pairwise-complete band the terms are those of its cells and its diagonal: the product with the windowed
        pairwise-complete matrix, which ld_matvec itself does not offer."""
        x32, e, squeeze = matvec_rhs(x, self.n_snps, power, check_finite, self.values.device)
        require_gpu()
        return LDProduct(self._matvec_launch(x32, power), e, x32, self.window, power, squeeze)


def ld_band(panel: PackedPanel, positions=None, window_bp: int = 1_000_000, window_snps: Optional[int] = None,
            path: Optional[str] = None, workspace: Optional[torch.Tensor] = None, check_positions: bool = True,
            dosage: bool = False, missing: Optional[str] = None) -> LDBand:
    """The windowed (band) LD matrix, kept: the signed r of every pair i > j with pos_i - pos_j <= window, 4 bytes per
    unordered pair, no threshold and no sort (include/ldx.h, ldx_ld_band_dev) -- ld_triangle(fmt="r32")'s cells bit for bit,
    written by the band kernel as it computes them.  Positions and window as for ld_score.  ``path``: 'fp4' (default) or
    'mfma' (the int8 band: identical bytes).  ``workspace``: a uint8 device tensor of ldx_ld_band_workspace_bytes() bytes to
    reuse.  ``dosage=True``: genotype-dosage r (ld_triangle(fmt="r32", dosage=True)'s cells; the FP4 band, an even n_hap).

    The layout is computed on the device; its total, offsets[n], is read back once to size ``values`` -- the call's only
    synchronisation (besides the check of a device tensor of positions, unless ``check_positions`` is False).

    ``missing="pairwise"``: the cells are the pairwise-complete r of ld_rect(panel, panel, missing="pairwise") at (i, j), bit
    for bit -- every pair over the haplotypes (``dosage``: the individuals) called at both SNPs -- at the cost of the band
    instead of the square (include/ldx.h, "pairwise-complete bands"; ldx_ld_pw_band_dev: the FP4 band only; ``workspace`` of
    ldx_ld_pw_band_workspace_bytes() bytes).  ``diag`` is +1 where the SNP is polymorphic among its own called observations,
    else -0.0.  A panel without missing codes gives the ``missing=None`` band bit for bit.  None: the call as it always was."""
    pairwise = _band_missing("ld_band", missing, path)
    if dosage:
        _dosage_check("ld_band", panel)
    require_gpu()
    n = panel.n_snps
    pos, pos_h, window = _band_positions(panel, positions, window_bp, window_snps, check_positions, "ld_band")
    window = min(window, BAND_WINDOW_MAX)
    if pairwise:
        return _pw_band(panel, pos, pos_h, window, workspace, bool(dosage), missing)
    pcode = _band_path(path)
    workspace = _band_workspace(lib.ldx_ld_band_workspace_bytes, panel, workspace)
    dev = panel.device
    lo, offsets, n_cells = _band_layout(pos, n, window, dev)
    values = torch.empty(n_cells, dtype=torch.float32, device=dev)
    if dosage:
        check(lib.ldx_ld_band_dosage_dev(*_dosage_panel(panel), n, panel.n_hap, pos.data_ptr(), window, pcode, lo.data_ptr(),
                                         offsets.data_ptr(), _ptr(values) if n_cells else None, n_cells, *_ws(workspace),
                                         _stream_ptr()), "ldx_ld_band_dosage_dev")
        live = panel.dosage_stats()[1][:n, 1] > 0.0
        diag = torch.where(live, torch.ones((), dtype=torch.float32, device=dev),
                           torch.full((), -0.0, dtype=torch.float32, device=dev))
    else:
        check(lib.ldx_ld_band_dev(*_phased_panel(panel), n, panel.n_hap, pos.data_ptr(), window, pcode, lo.data_ptr(),
                                  offsets.data_ptr(), _ptr(values) if n_cells else None, n_cells, *_ws(workspace),
                                  _stream_ptr()), "ldx_ld_band_dev")
        # r_matrix()'s diagonal (ldx_common.h, r32_diag): (n - a) / r in fp64, rounded to float32 once; -0.0f where a r == 0
        a, r = panel.acnt[:n].to(torch.float64), panel.rcnt[:n].to(torch.float64)
        live = (a * r) != 0
        quot = ((float(panel.n_hap) - a) / torch.where(live, r, torch.ones_like(r))).to(torch.float32)
        diag = torch.where(live, quot, torch.full((), -0.0, dtype=torch.float32, device=dev))
    res = LDBand(values, lo, offsets, diag.contiguous(), pos if pos_h is None else pos_h, window, bool(dosage), panel.n_hap)
    res._keep = (pos, workspace)   # alive until the launch is done
    return res


class CrossScores(np.ndarray):
    """ld_cross_score's result: a float64 [n] array (sums 2^-32) that also carries ``sums``, the exact int64 sums."""

    sums: np.ndarray


def ld_cross_score(band_a: LDBand, band_b: LDBand) -> np.ndarray:
    """Cross-panel LD scores from two stored bands that share a layout (same positions, same window; the panels may hold
    different haplotypes -- two populations' ``PackedPanel.select`` / ``split`` panels of one union panel -- and either band
    may be a dosage band): for every SNP i the sum of r1_ij r2_ij over the SNPs j with |pos_i - pos_j| <= window, i itself
    included (include/ldx.h, ldx_band_score_dev).  Every term is rint(2^32 (r1 *f32 r2)), added as a 64-bit integer: the
    result is reproducible and symmetric in its arguments.  Returns the scores as float64 [n] (sums 2^-32); the exact int64
    sums are its ``.sums``.  ``ld_cross_score(b, b)`` is ld_score's column 0, bit for bit.  Raises LdxError when the layouts
    differ.  Pairwise-complete bands (ld_band(missing="pairwise")) are bands like any other here: with two of them the
    result is the cross score of the pairwise-complete r, and ``ld_cross_score(b, b)`` is ld_score(missing="pairwise")'s
    column 0."""
    if not isinstance(band_a, LDBand) or not isinstance(band_b, LDBand):
        raise _lib.LdxError("ld_cross_score takes two LDBand results of ld_band")
    if not _same_layout(band_a, band_b):
        raise _lib.LdxError("ld_cross_score: the bands do not share a layout (same positions and the same window needed)")
    require_gpu()
    n = band_a.n_snps
    if band_a.values.device != band_b.values.device:
        raise _lib.LdxError("ld_cross_score: the bands live on different devices")
    sums = torch.empty(n, dtype=torch.int64, device=band_a.values.device)
    has = band_a.n_cells > 0
    check(lib.ldx_band_score_dev(_ptr(band_a.values) if has else None, _ptr(band_b.values) if has else None,
                                 band_a.diag.data_ptr(), band_b.diag.data_ptr(), band_a.lo.data_ptr(),
                                 band_a.offsets.data_ptr(), n, sums.data_ptr(), _stream_ptr()), "ldx_band_score_dev")
    sums_h = sums.cpu().numpy()
    out = (sums_h.astype(np.float64) / CROSS_SCALE).view(CrossScores)
    out.sums = sums_h
    return out


# --------------------------------------------------------------------------- neighbour lists, clumping, pruning
NONE_U32 = 0xFFFFFFFF            # rank of a SNP that is not a candidate; owner of a SNP without one (include/ldx.h)
SEL_INDEX, SEL_ASSIGNED, SEL_OUT = 1, 2, 3   # ldx_ld_select_dev's states (LDX_SEL_*)
SELECT_BATCH = 32                # selection rounds enqueued between two reads of the undecided count


def r2_bound(t: float, strict: bool = False) -> np.float32:
    """The float32 bound b of ldx_ld_neighbors_dev for a threshold t > 0: ``r^2 >= t`` is s >= b with b the smallest float32
    not below t, ``r^2 > t`` (strict) is s >= b with b the smallest float32 above t (s = r *f32 r is a float32)."""
    t = float(t)
    if not (0.0 < t < np.inf):
        raise _lib.LdxError(f"the r^2 threshold must be a finite number > 0 (got {t})")
    with np.errstate(over="ignore"):
        b = np.float32(t)
    if float(b) < t or (strict and float(b) == t):
        b = np.nextafter(b, np.float32(np.inf), dtype=np.float32)
    return np.float32(b)


def live_snps(acnt, rcnt) -> np.ndarray:
    """bool [n]: the SNP is not degenerate (a r > 0: it has ALT and REF codes)."""
    return np.asarray(acnt, dtype=np.int64) * np.asarray(rcnt, dtype=np.int64) > 0


def clump_ranks(pvalues, p1: float, p2: float, live) -> Tuple[np.ndarray, np.ndarray]:
    """(rank uint32 [n], member_ok uint8 [n]) of ld_clump: candidates are the SNPs with p <= p1, ranked by (p, row); members
    need p <= p2.  A SNP with a NaN p or a degenerate one (``live`` False) is neither.  Requires 0 < p1 <= p2."""
    p = np.asarray(pvalues, dtype=np.float64)
    live = np.asarray(live, dtype=bool)
    if p.ndim != 1 or p.shape != live.shape:
        raise _lib.LdxError(f"one p-value per SNP is needed ({live.size} SNPs, got shape {p.shape})")
    if not (0.0 < float(p1) <= float(p2)):
        raise _lib.LdxError(f"clumping needs 0 < p1 <= p2 (got p1 = {p1}, p2 = {p2})")
    if bool((p < 0).any()):
        raise _lib.LdxError("p-values must not be negative")
    ok = live & ~np.isnan(p)
    with np.errstate(invalid="ignore"):
        cand = ok & (p <= p1)
        member_ok = ok & (p <= p2)
    rows = np.flatnonzero(cand)
    order = rows[np.lexsort((rows, p[rows]))]
    rank = np.full(p.size, NONE_U32, dtype=np.uint32)
    rank[order] = np.arange(order.size, dtype=np.uint32)
    return rank, member_ok.astype(np.uint8)


def priority_ranks(priority, live) -> np.ndarray:
    """rank uint32 [n] of ld_prune: the live SNPs by priority, highest first, ties by row; UINT32_MAX for the others."""
    pr = np.asarray(priority, dtype=np.float64)
    live = np.asarray(live, dtype=bool)
    if pr.ndim != 1 or pr.shape != live.shape:
        raise _lib.LdxError(f"one priority per SNP is needed ({live.size} SNPs, got shape {pr.shape})")
    if bool(np.isnan(pr).any()):
        raise _lib.LdxError("priorities must not be NaN")
    rows = np.flatnonzero(live)
    order = rows[np.lexsort((rows, -pr[rows]))]
    rank = np.full(pr.size, NONE_U32, dtype=np.uint32)
    rank[order] = np.arange(order.size, dtype=np.uint32)
    return rank


def select_host(offsets, nbr, rank, member_ok) -> Tuple[np.ndarray, np.ndarray]:
    """The sequential rule ldx_ld_select_dev computes, as a plain loop (for small inputs and tests): take the candidates in
    increasing rank; one not yet assigned becomes an index, and each neighbour not yet assigned with member_ok set is
    assigned to it.  Returns (state uint8 [n]: SEL_INDEX / SEL_ASSIGNED / SEL_OUT, owner int64 [n]: -1 for none)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    nbr = np.asarray(nbr, dtype=np.int64)
    rank = np.asarray(rank, dtype=np.uint32)
    member_ok = np.asarray(member_ok).astype(bool)
    n = rank.size
    owner = np.full(n, -1, dtype=np.int64)
    state = np.where(rank == NONE_U32, SEL_OUT, SEL_ASSIGNED).astype(np.uint8)
    cands = np.flatnonzero(rank != NONE_U32)
    for i in cands[np.argsort(rank[cands], kind="stable")].tolist():
        if owner[i] >= 0:
            continue
        owner[i] = i
        state[i] = SEL_INDEX
        for j in nbr[offsets[i]:offsets[i + 1]].tolist():
            if owner[j] < 0 and member_ok[j]:
                owner[j] = i
    return state, owner


@dataclass
class LDNeighbors:
    """Per-SNP neighbour lists (ld_neighbors): for every SNP i the SNPs j != i with |pos_i - pos_j| <= window and r^2 above
    the threshold, as a CSR on the device.  ``hits`` holds the ldx_hit records (int32 [m, 4]: row, neighbour, r bits, s
    bits) sorted by (row, neighbour); row i's are [offsets[i], offsets[i + 1])."""

    offsets: torch.Tensor   # int32 [n + 1]
    hits: torch.Tensor      # int32 [m, 4]
    n_snps: int
    window: int
    bound: np.float32       # the float32 bound on s = r *f32 r (r2_bound)
    dosage: bool = False    # r is the genotype-dosage r (ld_neighbors(dosage=True))
    missing: Optional[str] = None   # "pairwise": r is the pairwise-complete r (ld_neighbors(missing="pairwise"))
    em: bool = False        # r is ld_em's r and column 3 of ``hits`` its D' cell, not s (ld_neighbors(em=True))

    @property
    def dprime(self) -> torch.Tensor:
        """float32 [m]: the D' cell of each pair of an EM list (a view of ``hits``)."""
        if not self.em:
            raise _lib.LdxError("these neighbour lists carry s = r *f32 r, not D': D' comes with ld_neighbors(em=True)")
        return self.hits[:, 3].view(torch.float32)

    @property
    def nbr(self) -> torch.Tensor:
        """int32 [m]: the neighbour rows (a view of ``hits``)."""
        return self.hits[:, 1]

    @property
    def r(self) -> torch.Tensor:
        """float32 [m]: the signed r of each (row, neighbour) pair -- the r32 cell, bit for bit (a view of ``hits``)."""
        return self.hits[:, 2].view(torch.float32)

    def __len__(self) -> int:
        return int(self.hits.shape[0])

    def pairs(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(i int64, j int64, r float32) on the host: every neighbour pair once, with i < j, sorted by (i, j)."""
        h = self.hits.cpu().numpy()
        i, j = h[:, 0].astype(np.int64), h[:, 1].astype(np.int64)
        once = i < j
        return i[once], j[once], h[once, 2].view(np.float32)


def ld_neighbors(panel: PackedPanel, positions=None, window_bp: int = 250_000, window_snps: Optional[int] = None,
                 r2: float = 0.2, strict: bool = False, path: Optional[str] = None, hit_capacity: Optional[int] = None,
                 workspace: Optional[torch.Tensor] = None, check_positions: bool = True, dosage: bool = False,
                 missing: Optional[str] = None, em: bool = False) -> LDNeighbors:
    """Neighbour lists on the matrix-pipe band (include/ldx.h, ldx_ld_neighbors_dev + ldx_area_finish_ex_dev): for every SNP
    the SNPs j with |pos_i - pos_j| <= window, j != i, and r^2 >= ``r2`` (``strict``: r^2 > r2), where r is the r32 cell of
    ld_triangle(fmt="r32") bit for bit and r^2 one float32 multiply.  Degenerate SNPs have no neighbours.

    Positions and window as for ld_score.  ``path``: 'fp4' (default) or 'mfma' (the int8 band: identical lists).
    ``hit_capacity``: record slots to start with (16 bytes each; default max(2^20, 32 n)); a call that needs more runs
    again at the count the first run reserved.  ``workspace``: a uint8 device tensor of ldx_ld_neighbors_workspace_bytes()
    bytes to reuse.  The host reads the record count once.

    ``dosage=True``: r is the genotype-dosage r of ld_triangle(fmt="r32", dosage=True), bit for bit (include/ldx.h,
    ldx_ld_neighbors_dosage_dev; the FP4 band only); SNPs whose dosage does not vary (v == 0) have no neighbours.

    ``missing="pairwise"``: r is the pairwise-complete r of ld_rect(missing="pairwise"), bit for bit -- what PLINK --r2 /
    --indep-pairwise compare with the threshold on a panel with missing calls (include/ldx.h, "pairwise-complete bands";
    ldx_ld_pw_neighbors_dev: the FP4 band only; ``workspace`` of ldx_ld_pw_band_workspace_bytes() bytes).  None: the call as
    it always was.

    ``em=True``: r is the EM r of ld_em(panel, panel, missing=missing), bit for bit -- the maximum-likelihood r of the unphased
    genotypes, PLINK --r2 / --clump's own; column 3 of the records is the D' cell (``.dprime``), not r^2 (include/ldx.h, "EM on
    the band"; ldx_ld_em_neighbors_dev: the FP4 band only, an even n_hap, not with ``dosage``; ``workspace`` of
    ldx_ld_em_band_workspace_bytes() bytes).  SNPs monomorphic among their called individuals have no neighbours; an
    all-heterozygous SNP can have some."""
    if em:
        return _em_neighbors(panel, positions, window_bp, window_snps, r2, strict, path, hit_capacity, workspace, check_positions,
                             dosage, missing)
    pairwise = _band_missing("ld_neighbors", missing, path)
    if dosage:
        _dosage_check("ld_neighbors", panel)
    require_gpu()
    n = panel.n_snps
    bound = r2_bound(r2, strict)
    pos, _, window = _band_positions(panel, positions, window_bp, window_snps, check_positions, "ld_neighbors")
    if pairwise:
        offsets, hits = _plan_neighbors("ldx_ld_pw_neighbors_dev", lib.ldx_ld_pw_band_workspace_bytes, panel,
                                        (*_pw_panel(panel, dosage), n, panel.n_hap, int(bool(dosage))), pos, window, bound,
                                        hit_capacity, workspace)
        return LDNeighbors(offsets, hits, n, window, bound, bool(dosage), missing)
    pcode = _band_path(path)
    workspace = _band_workspace(lib.ldx_ld_neighbors_workspace_bytes, panel, workspace)
    entry = "ldx_ld_neighbors_dosage_dev" if dosage else "ldx_ld_neighbors_dev"
    head = _dosage_panel(panel) if dosage else _phased_panel(panel)

    def launch(raw, cap, n_hits, counts):
        check(getattr(lib, entry)(*head, n, panel.n_hap, pos.data_ptr(), window, float(bound), pcode, raw.data_ptr(), cap,
                                  n_hits.data_ptr(), counts, *_ws(workspace), _stream_ptr()), entry)

    # the default capacity is max(2^20, 32 n): _rect_hits_run's with no panel J
    offsets, hits = _rect_hits_run("ld_neighbors", launch, n, 0, panel.device, hit_capacity, counts_ready=1)
    return LDNeighbors(offsets, hits, n, window, bound, bool(dosage))


def select_dev(nb: LDNeighbors, rank, member_ok, batch: int = SELECT_BATCH) -> Tuple[np.ndarray, np.ndarray, int]:
    """ldx_ld_select_dev over a neighbour CSR, in batches of ``batch`` rounds until no candidate is undecided.  Returns
    (state uint8 [n], owner int64 [n] with -1 for none, rounds enqueued).  More rounds than candidates raise LdxError."""
    n = nb.n_snps
    rank = np.ascontiguousarray(rank, dtype=np.uint32)
    member_ok = np.ascontiguousarray(member_ok, dtype=np.uint8)
    cand = rank != NONE_U32
    n_cand = int(cand.sum())
    if bool((cand & (member_ok == 0)).any()):
        raise _lib.LdxError("every candidate must have member_ok set")
    if n_cand and np.unique(rank[cand]).size != n_cand:
        raise _lib.LdxError("candidate ranks must be distinct")
    if n_cand == 0:
        return np.full(n, SEL_OUT, dtype=np.uint8), np.full(n, -1, dtype=np.int64), 0
    dev = nb.offsets.device
    ws_bytes = lib.ldx_ld_select_workspace_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    rank_d = torch.as_tensor(rank.view(np.int32)).to(dev)
    ok_d = torch.as_tensor(member_ok).to(dev)
    state = torch.empty(n, dtype=torch.uint8, device=dev)
    owner = torch.empty(n, dtype=torch.int32, device=dev)
    undecided = torch.empty(1, dtype=torch.int32, device=dev)
    nbrs = nb.hits.data_ptr() if len(nb) else None
    done = 0
    while True:
        check(lib.ldx_ld_select_dev(nbrs, nb.offsets.data_ptr(), n, rank_d.data_ptr(), ok_d.data_ptr(), done, int(batch),
                                    state.data_ptr(), owner.data_ptr(), undecided.data_ptr(), ws.data_ptr(), ws_bytes,
                                    _stream_ptr()), "ldx_ld_select_dev")
        done += int(batch)
        if int(undecided.item()) == 0:
            break
        if done >= n_cand:   # each round decides at least the lowest-ranked undecided candidate
            raise _lib.LdxError(f"selection left candidates undecided after {done} rounds ({n_cand} candidates)")
    own = owner.cpu().numpy().view(np.uint32)
    return state.cpu().numpy(), np.where(own == NONE_U32, -1, own.astype(np.int64)), done


@dataclass
class Clumps:
    """The clumps of ld_clump.  ``index``: the index rows in rank order (increasing p, then row); ``owner``: int64 [n], the
    index row each SNP belongs to (its own row for an index, -1 for none); ``nan_p`` / ``degenerate``: rows left out of
    clumping (neither candidates nor members)."""

    index: np.ndarray
    owner: np.ndarray
    nan_p: np.ndarray
    degenerate: np.ndarray
    neighbors: LDNeighbors
    rounds: int

    def members(self, index_row: int) -> np.ndarray:
        """int64: the rows assigned to this index (itself excluded), in row order."""
        return np.flatnonzero((self.owner == int(index_row)) & (np.arange(self.owner.size) != int(index_row)))

    def clumps(self):
        """[(index row, member rows)] in rank order."""
        return [(int(k), self.members(k)) for k in self.index]


@dataclass
class Pruned:
    """The result of ld_prune: ``keep`` bool [n] (no two kept SNPs are neighbours), and the ranks it used."""

    keep: np.ndarray
    rank: np.ndarray
    neighbors: LDNeighbors
    rounds: int


def _panel_live(panel: PackedPanel, dosage: bool = False, pairwise: bool = False, em: bool = False) -> np.ndarray:
    """The SNPs that can have a neighbour: a r > 0, or for the dosage lists v > 0 (pairwise-complete: v over the individuals
    called at the SNP); for the EM lists 0 < A < 2 N over the SNP's called individuals (em_snp_stats)."""
    if em:
        return em_snp_stats(panel, pairwise)[3].cpu().numpy().astype(bool)
    if pairwise and dosage:
        return pw_snp_stats(panel, True)[1].cpu().numpy().astype(bool)
    return panel.dosage_live() if dosage else live_snps(panel.alt_counts(), panel.ref_counts())


def ld_clump(panel: PackedPanel, positions, pvalues, p1: float = 1e-4, p2: float = 1e-2, r2: float = 0.5,
             window_bp: int = 250_000, window_snps: Optional[int] = None, path: Optional[str] = None,
             hit_capacity: Optional[int] = None, dosage: bool = False, missing: Optional[str] = None,
             em: bool = False) -> Clumps:
    """Clumping (PLINK --clump's rule): take the SNPs with p <= p1 in increasing (p, row); one not yet in a clump becomes an
    index and takes every SNP not yet in a clump with p <= p2 and r^2 >= r2 within the window.  r^2 is that of ld_neighbors
    (the haplotype r of the ALT indicators, unrounded; ``dosage=True``: the genotype-dosage r, PLINK's own).  SNPs with a
    NaN p and degenerate SNPs (dosage: v == 0) take no part.  ``missing="pairwise"``: ld_neighbors(missing="pairwise")'s
    lists -- r^2 over the observations called at both SNPs.  ``em=True``: ld_neighbors(em=True)'s lists -- the EM r^2 of the
    unphased genotypes; with ``missing="pairwise"`` PLINK --clump's own r^2.  SNPs monomorphic among their called individuals
    take no part; an all-heterozygous SNP does."""
    pairwise = _em_args("ld_clump", panel, missing, path, dosage) if em else _band_missing("ld_clump", missing, path)
    if dosage:
        _dosage_check("ld_clump", panel)
    live = _panel_live(panel, dosage, pairwise, em)
    rank, member_ok = clump_ranks(pvalues, p1, p2, live)
    nb = ld_neighbors(panel, positions, window_bp=window_bp, window_snps=window_snps, r2=r2, strict=False, path=path,
                      hit_capacity=hit_capacity, dosage=dosage, missing=missing, em=em)
    state, owner, rounds = select_dev(nb, rank, member_ok)
    idx = np.flatnonzero(state == SEL_INDEX)
    idx = idx[np.argsort(rank[idx], kind="stable")]
    p = np.asarray(pvalues, dtype=np.float64)
    return Clumps(idx.astype(np.int64), owner, np.flatnonzero(np.isnan(p)), np.flatnonzero(~live), nb, rounds)


def ld_prune(panel: PackedPanel, positions=None, r2: float = 0.2, window_bp: Optional[int] = None,
             window_snps: Optional[int] = None, priority=None, path: Optional[str] = None,
             hit_capacity: Optional[int] = None, dosage: bool = False, missing: Optional[str] = None,
             em: bool = False) -> Pruned:
    """Priority pruning: take the SNPs in decreasing priority (default: the MAF min(fa, fr) of the panel), ties by row; one
    with no kept neighbour is kept.  Neighbours are the SNPs within the window with r^2 > r2 (strict), as in ld_neighbors.
    The kept set has no pair above the threshold inside the window.  Degenerate SNPs are never kept.  The window is
    ``window_snps`` SNPs or ``window_bp`` in the units of ``positions`` (default 250 000 when positions are given).
    ``dosage=True``: the neighbours are those of the genotype-dosage r (PLINK --indep-pairwise's r), SNPs with v == 0 are
    never kept, and the default priority is the dosage MAF min(f, 1 - f), f = a / n_hap.  ``missing="pairwise"``:
    ld_neighbors(missing="pairwise")'s lists -- PLINK --indep-pairwise's r^2 on a panel with missing calls.  ``em=True``:
    ld_neighbors(em=True)'s lists; SNPs monomorphic among their called individuals are never kept, and the default priority is
    min(f, 1 - f) with f = A / (2 N) over the SNP's called individuals (em_snp_stats)."""
    pairwise = _em_args("ld_prune", panel, missing, path, dosage) if em else _band_missing("ld_prune", missing, path)
    if dosage:
        _dosage_check("ld_prune", panel)
    live = _panel_live(panel, dosage, pairwise, em)
    if priority is None and em:
        n_called, a_sum = (t.cpu().numpy().astype(np.float64) for t in em_snp_stats(panel, pairwise)[:2])
        f = a_sum / np.maximum(2.0 * n_called, 1.0)
        priority = np.minimum(f, 1.0 - f)
    if priority is None and dosage:
        f = panel.fa.cpu().numpy()[:panel.n_snps]
        priority = np.minimum(f, 1.0 - f)
    if priority is None:
        priority = np.minimum(panel.fa.cpu().numpy()[:panel.n_snps], panel.fr.cpu().numpy()[:panel.n_snps])
    rank = priority_ranks(priority, live)
    if window_snps is None and window_bp is None:
        window_bp = 250_000
    nb = ld_neighbors(panel, positions, window_bp=0 if window_bp is None else window_bp, window_snps=window_snps, r2=r2,
                      strict=True, path=path, hit_capacity=hit_capacity, dosage=dosage, missing=missing, em=em)
    state, _, rounds = select_dev(nb, rank, live.astype(np.uint8))
    return Pruned(state == SEL_INDEX, rank, nb, rounds)


# --------------------------------------------------------------------------- rectangular LD (two SNP sets)
def _rect_panels(what: str, panel_i: PackedPanel, panel_j: Optional[PackedPanel], dosage: bool) -> PackedPanel:
    """The rectangle's argument rules, checked before anything touches the device; returns panel J."""
    pj = panel_i if panel_j is None else panel_j
    if not isinstance(panel_i, PackedPanel) or not isinstance(pj, PackedPanel):
        raise _lib.LdxError(f"{what}: panel_i and panel_j must be PackedPanels")
    if pj.n_hap != panel_i.n_hap:
        raise _lib.LdxError(f"{what}: the panels differ in haplotype count (n_hap {panel_i.n_hap} and {pj.n_hap}): "
                            "the rectangle pairs SNPs over the SAME haplotypes")
    if pj.device != panel_i.device:
        raise _lib.LdxError(f"{what}: the panels are on different devices ({panel_i.device} and {pj.device})")
    if dosage and panel_i.n_hap % 2:
        raise _lib.LdxError(f"{what}: dosage=True needs an even n_hap (got {panel_i.n_hap}): individual k owns haplotypes "
                            "2k and 2k + 1")
    return pj


def _rect_out(what: str, name: str, out, n_i: int, n_j: int, dev):
    """An output matrix of ld_rect / ld_em: a float32 [n_i, >= n_j] tensor with unit column stride on ``dev``; returns
    (tensor, row stride)."""
    if (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != n_i
            or out.shape[1] < n_j or (out.shape[1] > 1 and out.stride(1) != 1) or out.device != dev):
        raise _lib.LdxError(f"{what}: {name} must be a float32 [{n_i}, >= {n_j}] tensor with unit column stride on {dev}")
    ld = out.stride(0) if n_i > 1 else max(out.stride(0), out.shape[1])
    if ld < n_j:
        raise _lib.LdxError(f"{what}: {name} has row stride {ld} < n_j = {n_j}")
    return out, ld


def _rect_side(panel: PackedPanel, dosage: bool) -> tuple:
    """One side's arguments of the rectangle entries: alt, gstat, n (dosage) or alt, acnt, rcnt, n."""
    if dosage:
        return (*_dosage_panel(panel), panel.n_snps)
    return panel.alt.data_ptr(), panel.acnt.data_ptr(), panel.rcnt.data_ptr(), panel.n_snps


def _rect_missing(what: str, missing) -> bool:
    """The rectangle's ``missing`` argument: None (the operator's own rule) or "pairwise" (pairwise-complete); True for the
    latter.  Anything else is refused before the device is touched."""
    if missing is None:
        return False
    if isinstance(missing, str) and missing == "pairwise":
        return True
    raise _lib.LdxError(f'{what}: missing must be None or "pairwise", got {missing!r}')


def _pw_side(panel: PackedPanel) -> tuple:
    """One side's arguments of the pairwise-complete entries: alt, ref, acnt, rcnt, n."""
    return panel.alt.data_ptr(), panel.ref.data_ptr(), panel.acnt.data_ptr(), panel.rcnt.data_ptr(), panel.n_snps


# ---- pairwise-complete bands (include/ldx.h, "pairwise-complete bands")
def _band_missing(what: str, missing, path) -> bool:
    """The band operators' ``missing`` argument (_rect_missing's rule); "pairwise" runs on the FP4 band only.  Checked before
    anything touches the device."""
    pairwise = _rect_missing(what, missing)
    if pairwise and path not in (None, "fp4"):
        raise _lib.LdxError(f'{what}: missing="pairwise" runs on the FP4 band only (path must be None or \'fp4\', got {path!r})')
    return pairwise


def _pw_panel(panel: PackedPanel, dosage: bool) -> tuple:
    """The panel's arguments of the pairwise-complete band entries: alt, ref, acnt, rcnt, hom (None unless ``dosage``)."""
    hom = panel.dosage_stats()[0].data_ptr() if dosage else None
    return panel.alt.data_ptr(), panel.ref.data_ptr(), panel.acnt.data_ptr(), panel.rcnt.data_ptr(), hom


def pw_snp_stats(panel: PackedPanel, dosage: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(diag float32 [n], live uint8 [n])`` on the device: the diagonal of a pairwise-complete band and what it stands on
    (include/ldx.h, ldx_pw_snp_stats_dev) -- the SNP is polymorphic over its OWN called set: a r > 0, or with ``dosage``
    N (A + 2 HA) - A^2 > 0 over the individuals with both codes called; diag is +1.0 where live, else -0.0."""
    require_gpu()
    n = panel.n_snps
    diag = torch.empty(n, dtype=torch.float32, device=panel.device)
    live = torch.empty(n, dtype=torch.uint8, device=panel.device)
    check(lib.ldx_pw_snp_stats_dev(panel.alt.data_ptr(), panel.ref.data_ptr(), panel.acnt.data_ptr(), panel.rcnt.data_ptr(), n,
                                   panel.n_hap, int(bool(dosage)), diag.data_ptr(), live.data_ptr(), _stream_ptr()),
          "ldx_pw_snp_stats_dev")
    return diag, live


def _pw_band(panel: PackedPanel, pos, pos_h, window: int, workspace, dosage: bool, missing) -> "LDBand":
    """ld_band(missing="pairwise") after the argument checks: ld_band's layout, ldx_ld_pw_band_dev's cells."""
    n, dev = panel.n_snps, panel.device
    workspace = _plan_workspace(lib.ldx_ld_pw_band_workspace_bytes, panel, workspace)
    lo, offsets, n_cells = _band_layout(pos, n, window, dev)
    values = torch.empty(n_cells, dtype=torch.float32, device=dev)
    check(lib.ldx_ld_pw_band_dev(*_pw_panel(panel, dosage), n, panel.n_hap, int(dosage), pos.data_ptr(), window, lo.data_ptr(),
                                 offsets.data_ptr(), _ptr(values) if n_cells else None, n_cells, *_ws(workspace), _stream_ptr()),
          "ldx_ld_pw_band_dev")
    diag, _ = pw_snp_stats(panel, dosage)
    res = LDBand(values, lo, offsets, diag, pos if pos_h is None else pos_h, window, dosage, panel.n_hap, missing=missing)
    res._keep = (pos, workspace)   # alive until the launch is done
    return res


def ld_rect(panel_i: PackedPanel, panel_j: Optional[PackedPanel] = None, dosage: bool = False,
            out: Optional[torch.Tensor] = None, missing: Optional[str] = None) -> torch.Tensor:
    """Signed r of every SNP of ``panel_i`` against every SNP of ``panel_j`` (None: ``panel_i`` itself, the full square) over
    the same haplotypes: float32 [n_i, n_j] on the device (include/ldx.h, ldx_ld_rect_dev).  Cell (i, j) is the r32 cell of
    ld_triangle(fmt="r32") for those two SNPs bit for bit -- -0.0f on a degenerate pair, +0.0f iff the covariance is 0 --
    also where the two rows are the same variant (the pair formula, not the triangle's one-division diagonal).  The two
    panels are typically ``PackedPanel.select(snps=...)`` sub-panels of one panel, or two chromosomes of one sample set.

    ``dosage=True``: the genotype-dosage r of ld_triangle(fmt="r32", dosage=True) (even n_hap).  ``out``: a float32 device
    tensor [n_i, >= n_j] with unit column stride to write into; its row stride is taken as it is and the columns beyond n_j
    are left untouched.  The view out[:, :n_j] is returned.

    ``missing="pairwise"``: pairwise-complete r (include/ldx.h, "pairwise-complete LD"; ldx_ld_rect_pw_dev) -- every pair over
    the haplotypes (``dosage``: the individuals, a half-missing genotype being missing) called at both SNPs, as PLINK --r2
    does.  A pair of rows without missing codes gives the ``missing=None`` cell bit for bit.  None: the call as it always was
    (n is every haplotype and the allele counts leave a hole out; ``dosage`` counts it as REF)."""
    pairwise = _rect_missing("ld_rect", missing)
    pj = _rect_panels("ld_rect", panel_i, panel_j, dosage)
    n_i, n_j = panel_i.n_snps, pj.n_snps
    if out is not None:
        out, ld_out = _rect_out("ld_rect", "out", out, n_i, n_j, panel_i.device)
    require_gpu()
    if out is None:
        out = torch.empty((n_i, n_j), dtype=torch.float32, device=panel_i.device)
        ld_out = n_j
    if pairwise:
        check(lib.ldx_ld_rect_pw_dev(*_pw_side(panel_i), *_pw_side(pj), panel_i.n_hap, int(bool(dosage)), out.data_ptr(),
                                     ld_out, _stream_ptr()), "ldx_ld_rect_pw_dev")
        return out[:, :n_j]
    entry = "ldx_ld_rect_dosage_dev" if dosage else "ldx_ld_rect_dev"
    check(getattr(lib, entry)(*_rect_side(panel_i, dosage), *_rect_side(pj, dosage), panel_i.n_hap, out.data_ptr(), ld_out,
                              _stream_ptr()), entry)
    return out[:, :n_j]


def rect_hits_host(r, bound) -> Tuple[np.ndarray, np.ndarray]:
    """Host mirror of ldx_ld_rect_hits_dev's rule on a float32 matrix ``r`` of r32 cells: the (i, j), as two int64 arrays in
    (i, j) order, with ``np.multiply(r, r, dtype=np.float32) >= bound`` and r not -0.0f (a degenerate pair is never a hit,
    whatever the bound)."""
    r = np.asarray(r)
    if r.dtype != np.float32 or r.ndim != 2:
        raise _lib.LdxError(f"rect_hits_host: r must be a float32 matrix, got {r.dtype} with shape {r.shape}")
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.multiply(r, r, dtype=np.float32)
        keep = (s >= np.float32(bound)) & (r.view(np.uint32) != np.uint32(0x80000000))
    i, j = np.nonzero(keep)   # row-major: sorted by (i, j)
    return i.astype(np.int64), j.astype(np.int64)


@dataclass
class LDRectHits:
    """The pairs of a rectangle above an r^2 threshold (ld_rect_hits) as a CSR over the rows of panel I, on the device.
    ``hits`` holds the ldx_hit records (int32 [m, 4]: i, j, r bits, s bits with s = r *f32 r) sorted by (i, j); row i's are
    [offsets[i], offsets[i + 1])."""

    offsets: torch.Tensor   # int32 [n_i + 1]
    hits: torch.Tensor      # int32 [m, 4]
    n_i: int
    n_j: int
    bound: np.float32       # the float32 bound on s (r2_bound)
    dosage: bool = False
    em: bool = False        # ld_em_hits: r is the EM r and column 3 of ``hits`` the D' cell instead of s
    missing: Optional[str] = None   # "pairwise": the cells are ld_rect(missing="pairwise")'s (``em``: ld_em(missing="pairwise")'s)

    @property
    def j(self) -> torch.Tensor:
        """int32 [m]: the panel-J rows (a view of ``hits``)."""
        return self.hits[:, 1]

    @property
    def r(self) -> torch.Tensor:
        """float32 [m]: the signed r of each pair -- the ld_rect cell, bit for bit (a view of ``hits``)."""
        return self.hits[:, 2].view(torch.float32)

    @property
    def dprime(self) -> torch.Tensor:
        """float32 [m]: the D' of each pair -- the ld_em cell, bit for bit (ld_em_hits only; a view of ``hits``)."""
        if not self.em:
            raise _lib.LdxError("LDRectHits.dprime: only ld_em_hits records carry D'")
        return self.hits[:, 3].view(torch.float32)

    def __len__(self) -> int:
        return int(self.hits.shape[0])

    def pairs(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(i int64, j int64, r float32) on the host, sorted by (i, j)."""
        h = self.hits.cpu().numpy()
        return h[:, 0].astype(np.int64), h[:, 1].astype(np.int64), np.ascontiguousarray(h[:, 2]).view(np.float32)


def ld_rect_hits(panel_i: PackedPanel, panel_j: Optional[PackedPanel] = None, r2: float = 0.2, strict: bool = False,
                 dosage: bool = False, hit_capacity: Optional[int] = None, missing: Optional[str] = None) -> LDRectHits:
    """The pairs (row i of ``panel_i``, row j of ``panel_j``) with r^2 >= ``r2`` (``strict``: r^2 > r2), where r is the
    ld_rect cell bit for bit and r^2 one float32 multiply -- ld_neighbors' rule without a window, once per (i, j)
    (include/ldx.h, ldx_ld_rect_hits_dev + ldx_area_finish_ex_dev).  Degenerate pairs are never hits.

    ``hit_capacity``: record slots to start with (16 bytes each; default max(2^20, 32 (n_i + n_j))); a call that needs more
    runs again at the count the first run reserved plus ld_neighbors' margin, at most four times.  The host reads the
    record count once per run.  ``missing="pairwise"``: r is the ld_rect(missing="pairwise") cell (ldx_ld_rect_pw_hits_dev)."""
    pairwise = _rect_missing("ld_rect_hits", missing)
    pj = _rect_panels("ld_rect_hits", panel_i, panel_j, dosage)
    bound = r2_bound(r2, strict)
    require_gpu()
    n_i, n_j = panel_i.n_snps, pj.n_snps

    entry = "ldx_ld_rect_hits_dosage_dev" if dosage else "ldx_ld_rect_hits_dev"

    def launch(raw, cap, n_hits, _counts):
        if pairwise:
            check(lib.ldx_ld_rect_pw_hits_dev(*_pw_side(panel_i), *_pw_side(pj), panel_i.n_hap, int(bool(dosage)), float(bound),
                                              raw.data_ptr(), cap, n_hits.data_ptr(), _stream_ptr()), "ldx_ld_rect_pw_hits_dev")
            return
        check(getattr(lib, entry)(*_rect_side(panel_i, dosage), *_rect_side(pj, dosage), panel_i.n_hap, float(bound),
                                  raw.data_ptr(), cap, n_hits.data_ptr(), _stream_ptr()), entry)

    offsets, hits = _rect_hits_run("ld_rect_hits", launch, n_i, n_j, panel_i.device, hit_capacity)
    return LDRectHits(offsets, hits, n_i, n_j, bound, bool(dosage), missing=missing)


PAIRWISE_COUNTS = {False: ("n", "a", "b", "c"), True: ("N", "A", "B", "HA", "HB", "S")}   # the order of include/ldx.h


def ld_rect_counts(panel_i: PackedPanel, panel_j: Optional[PackedPanel] = None, dosage: bool = False) -> torch.Tensor:
    """The integers of every pair of pairwise-complete LD as the kernel's K loop produced them, before any float: uint32
    [4, n_i, n_j] (n, a, b, c) or, ``dosage``, [6, n_i, n_j] (N, A, B, HA, HB, S) on the device (include/ldx.h,
    ldx_ld_rect_pw_counts_dev)."""
    pj = _rect_panels("ld_rect_counts", panel_i, panel_j, dosage)
    require_gpu()
    n_i, n_j = panel_i.n_snps, pj.n_snps
    out = torch.empty((len(PAIRWISE_COUNTS[bool(dosage)]), n_i, n_j), dtype=torch.int32, device=panel_i.device)
    check(lib.ldx_ld_rect_pw_counts_dev(*_pw_side(panel_i), *_pw_side(pj), panel_i.n_hap, int(bool(dosage)), out.data_ptr(), n_j,
                                        _stream_ptr()), "ldx_ld_rect_pw_counts_dev")
    return out.view(torch.uint32)


def pairwise_counts_host(codes_i, codes_j, dosage: bool = False) -> np.ndarray:
    """Host mirror of the pairwise-complete counts (include/ldx.h, "pairwise-complete LD") in pure numpy: int64 [4, n_i, n_j]
    (n, a, b, c) over the jointly called haplotypes or, ``dosage``, [6, n_i, n_j] (N, A, B, HA, HB, S) over the individuals
    called at both SNPs (both codes of haplotypes 2k and 2k + 1 in {0, 1}).  float64 GEMMs of 0/1/2 matrices: exact."""
    ci, cj = np.asarray(codes_i), np.asarray(codes_j)
    if ci.ndim != 2 or cj.ndim != 2 or ci.shape[1] != cj.shape[1]:
        raise _lib.LdxError(f"pairwise_counts_host: two code matrices over the same haplotypes needed, got shapes {ci.shape} "
                            f"and {cj.shape}")
    if dosage and ci.shape[1] % 2:
        raise _lib.LdxError(f"pairwise_counts_host: dosage=True needs an even n_hap (got {ci.shape[1]})")

    def planes(c):
        alt, called = c == 1, (c == 0) | (c == 1)
        if not dosage:
            return called.astype(np.float64), alt.astype(np.float64), None
        q = called[:, 0::2] & called[:, 1::2]
        g = (alt[:, 0::2].astype(np.int64) + alt[:, 1::2].astype(np.int64)) * q
        return q.astype(np.float64), g.astype(np.float64), (g == 2).astype(np.float64)

    (qi, gi, hi), (qj, gj, hj) = planes(ci), planes(cj)
    if dosage:
        sets = [qi @ qj.T, gi @ qj.T, qi @ gj.T, hi @ qj.T, qi @ hj.T, gi @ gj.T]
    else:
        sets = [qi @ qj.T, gi @ qj.T, qi @ gj.T, gi @ gj.T]
    return np.stack(sets).astype(np.int64)


def pairwise_cell_host(counts, dosage: bool = False) -> np.ndarray:
    """Host mirror of the pairwise-complete cell (include/ldx.h): float32, the shape of one set, from the integers ``counts``
    [4 or 6, ...] in float64 with every operation rounded once -- -0.0f where either variance is 0, +0.0f where num = 0."""
    k = np.asarray(counts)
    want = len(PAIRWISE_COUNTS[bool(dosage)])
    if k.shape[0] != want:
        raise _lib.LdxError(f"pairwise_cell_host: {want} count sets needed (dosage={bool(dosage)}), got {k.shape[0]}")
    k = k.astype(np.float64)
    if dosage:
        N, A, B, HA, HB, S = k
        num = S * N - A * B                  # every product and the difference are integers below 2^53: exact, as the fma is
        vx, vy = N * (A + 2.0 * HA) - A * A, N * (B + 2.0 * HB) - B * B
    else:
        n, a, b, c = k
        num = c * n - a * b
        vx, vy = a * (n - a), b * (n - b)
    with np.errstate(divide="ignore", invalid="ignore"):
        rsx = np.where(vx > 0.0, 1.0 / np.sqrt(np.where(vx > 0.0, vx, 1.0)), 0.0)
        rsy = np.where(vy > 0.0, 1.0 / np.sqrt(np.where(vy > 0.0, vy, 1.0)), 0.0)
    s = rsx * rsy
    return np.where(s == 0.0, np.float32(-0.0), (num * s).astype(np.float32)).astype(np.float32)


def _rect_hits_run(what: str, launch, n_i: int, n_j: int, dev, hit_capacity: Optional[int], counts_ready: int = 0):
    """The hit entries' buffers and retry loop: ``launch(raw, cap, n_hits, counts)`` enqueues one run into ``cap`` record slots,
    ldx_area_finish_ex_dev sorts what it stored into a CSR over the rows of panel I; a run that reserved more slots than it
    had runs again at the reserved count plus a margin, at most four times.  ``counts_ready`` = 1 (ld_neighbors' band, which
    counts per row as it stores: no counting pass): ``counts`` is where the finishing step expects those counts
    (ldx_area_finish_counts); 0: ``counts`` is None and the finishing step counts the stored records per row itself.
    Returns (offsets, sorted records)."""
    fin_bytes = lib.ldx_area_finish_workspace_bytes(n_i)
    fin = torch.empty(fin_bytes, dtype=torch.uint8, device=dev)
    counts = lib.ldx_area_finish_counts(fin.data_ptr()) if counts_ready else None
    cap = int(hit_capacity) if hit_capacity is not None else max(1 << 20, 32 * (n_i + n_j))
    n_hits = torch.zeros(1, dtype=torch.int64, device=dev)
    summary = torch.zeros(2, dtype=torch.int64, device=dev)
    offsets = torch.empty(n_i + 1, dtype=torch.int32, device=dev)
    for attempt in range(4):
        if not 0 <= cap < (1 << 32):
            raise _lib.LdxError(f"{what}: {cap} record slots needed; the CSR's offsets are uint32 (at most 2^32 - 1)")
        raw = torch.empty((cap, 4), dtype=torch.int32, device=dev)
        hits = torch.empty((cap, 4), dtype=torch.int32, device=dev)
        launch(raw, cap, n_hits, counts)
        check(lib.ldx_area_finish_ex_dev(raw.data_ptr(), n_hits.data_ptr(), cap, n_i, hits.data_ptr(), offsets.data_ptr(),
                                         summary.data_ptr(), fin.data_ptr(), fin_bytes, counts_ready, _stream_ptr()),
              "ldx_area_finish_ex_dev")
        total, reserved = (int(x) for x in summary.tolist())
        if reserved <= cap:
            break
        # the slots the run reserved (records + the batches' unused tails): the count a re-run needs, give or take the tails
        # of a different work order -- hence the margin and, in the worst case, another run
        cap = reserved + reserved // 64 + (1 << 16)
    else:
        raise _lib.LdxError(f"{what}: the record count did not settle")
    del raw
    return offsets, hits[:total]


def _plan_neighbors(entry: str, size_fn, panel: PackedPanel, head: tuple, pos, window: int, bound, hit_capacity, workspace):
    """A plan band's neighbours entry (``entry``: ldx_ld_pw_neighbors_dev or ldx_ld_em_neighbors_dev, ``head`` its arguments in
    front of the positions) through _rect_hits_run, with ld_neighbors' default capacity.  Returns (offsets, sorted records)."""
    n = panel.n_snps
    workspace = _plan_workspace(size_fn, panel, workspace)

    def launch(raw, cap, n_hits, _counts):
        check(getattr(lib, entry)(*head, pos.data_ptr(), min(window, BAND_WINDOW_MAX), float(bound), raw.data_ptr(), cap,
                                  n_hits.data_ptr(), *_ws(workspace), _stream_ptr()), entry)

    cap = int(hit_capacity) if hit_capacity is not None else max(1 << 20, 32 * n)
    return _rect_hits_run("ld_neighbors", launch, n, 0, panel.device, cap)


# --------------------------------------------------------------------------- unphased LD by EM (two SNP sets)
@dataclass
class LDEm:
    """ld_em's two matrices on the device, float32 [n_i, n_j] each (None where only the other was asked for)."""

    r: Optional[torch.Tensor]
    dprime: Optional[torch.Tensor]


def ld_em(panel_i: PackedPanel, panel_j: Optional[PackedPanel] = None, out_r=None, out_dprime=None,
          want_r: bool = True, want_dprime: bool = True, missing: Optional[str] = None) -> LDEm:
    """Unphased LD by maximum likelihood of every SNP of ``panel_i`` against every SNP of ``panel_j`` (None: ``panel_i``
    itself) over the same individuals (even n_hap; individual k owns haplotypes 2k and 2k + 1): the EM haplotype frequency of
    the genotype table, and from it ``.r`` and ``.dprime``, float32 [n_i, n_j] on the device (include/ldx.h, "unphased LD by
    EM", ldx_ld_em_rect_dev) -- what PLINK --r2 dprime computes.  -0.0f in both on a degenerate pair; D' >= 0, the sign lives
    in r.

    ``out_r`` / ``out_dprime``: float32 device tensors [n_i, >= n_j] with unit column stride and one row stride to write into;
    the columns beyond n_j are left untouched.  ``want_r`` / ``want_dprime`` = False leaves that matrix out (None in the
    result); not both.

    ``missing="pairwise"``: every pair over the individuals called at BOTH SNPs (both codes of the individual 0 or 1: a
    half-missing genotype is missing), as PLINK --r2 dprime and Haploview treat missing calls -- the pair's own N, A = sum g_x,
    B = sum g_y, S and H through the same epilogue (include/ldx.h, "pairwise-complete EM"; ldx_ld_em_rect_pw_dev).  A pair of
    rows without missing codes gives the ``missing=None`` cell bit for bit; -0.0f in both where the joint set is empty or
    either SNP is monomorphic within it.  None: the call as it always was (a missing code counts as REF)."""
    pairwise = _rect_missing("ld_em", missing)
    pj = _rect_panels("ld_em", panel_i, panel_j, True)
    n_i, n_j, dev = panel_i.n_snps, pj.n_snps, panel_i.device
    if not ((want_r or out_r is not None) or (want_dprime or out_dprime is not None)):
        raise _lib.LdxError("ld_em: neither r nor D' was asked for")
    lds = []
    if out_r is not None:
        out_r, ld = _rect_out("ld_em", "out_r", out_r, n_i, n_j, dev)
        lds.append(ld)
    if out_dprime is not None:
        out_dprime, ld = _rect_out("ld_em", "out_dprime", out_dprime, n_i, n_j, dev)
        lds.append(ld)
    if len(set(lds)) > 1:
        raise _lib.LdxError(f"ld_em: out_r and out_dprime differ in row stride ({lds[0]} and {lds[1]}); the entry takes one")
    require_gpu()
    ld = lds[0] if lds else n_j
    if out_r is None and want_r:
        out_r = torch.empty((n_i, ld), dtype=torch.float32, device=dev)
    if out_dprime is None and want_dprime:
        out_dprime = torch.empty((n_i, ld), dtype=torch.float32, device=dev)
    outs = (out_r.data_ptr() if out_r is not None else None, out_dprime.data_ptr() if out_dprime is not None else None)
    if pairwise:
        check(lib.ldx_ld_em_rect_pw_dev(*_pw_side(panel_i), *_pw_side(pj), panel_i.n_hap, *outs, ld, _stream_ptr()),
              "ldx_ld_em_rect_pw_dev")
    else:
        check(lib.ldx_ld_em_rect_dev(panel_i.alt.data_ptr(), panel_i.acnt.data_ptr(), n_i, pj.alt.data_ptr(), pj.acnt.data_ptr(),
                                     n_j, panel_i.n_hap, *outs, ld, _stream_ptr()), "ldx_ld_em_rect_dev")
    return LDEm(out_r[:, :n_j] if out_r is not None else None, out_dprime[:, :n_j] if out_dprime is not None else None)


def ld_em_hits(panel_i: PackedPanel, panel_j: Optional[PackedPanel] = None, r2: float = 0.2, strict: bool = False,
               hit_capacity: Optional[int] = None, missing: Optional[str] = None) -> LDRectHits:
    """The pairs (row i of ``panel_i``, row j of ``panel_j``) whose EM r has r^2 >= ``r2`` (``strict``: r^2 > r2): r the ld_em
    cell bit for bit, r^2 one float32 multiply (include/ldx.h, ldx_ld_em_rect_hits_dev + ldx_area_finish_ex_dev).  The result
    is ld_rect_hits' CSR with ``em`` set: column 3 of ``hits`` holds the D' cell (``.dprime``).  Buffers and retries are
    ld_rect_hits'.  ``missing="pairwise"``: the cells are ld_em(missing="pairwise")'s (ldx_ld_em_rect_pw_hits_dev)."""
    pairwise = _rect_missing("ld_em_hits", missing)
    pj = _rect_panels("ld_em_hits", panel_i, panel_j, True)
    bound = r2_bound(r2, strict)
    require_gpu()
    n_i, n_j = panel_i.n_snps, pj.n_snps

    def launch(raw, cap, n_hits, _counts):
        if pairwise:
            check(lib.ldx_ld_em_rect_pw_hits_dev(*_pw_side(panel_i), *_pw_side(pj), panel_i.n_hap, float(bound), raw.data_ptr(),
                                                 cap, n_hits.data_ptr(), _stream_ptr()), "ldx_ld_em_rect_pw_hits_dev")
            return
        check(lib.ldx_ld_em_rect_hits_dev(panel_i.alt.data_ptr(), panel_i.acnt.data_ptr(), n_i, pj.alt.data_ptr(),
                                          pj.acnt.data_ptr(), n_j, panel_i.n_hap, float(bound), raw.data_ptr(), cap,
                                          n_hits.data_ptr(), _stream_ptr()), "ldx_ld_em_rect_hits_dev")

    offsets, hits = _rect_hits_run("ld_em_hits", launch, n_i, n_j, panel_i.device, hit_capacity)
    return LDRectHits(offsets, hits, n_i, n_j, bound, False, True, missing=missing)


# ---- EM on the band (include/ldx.h, "EM on the band")
def _em_args(what: str, panel: PackedPanel, missing, path=None, dosage: bool = False) -> bool:
    """The EM band operators' argument rules, checked before anything touches the device; True for missing="pairwise"."""
    pairwise = _rect_missing(what, missing)
    if dosage:
        raise _lib.LdxError(f"{what}: em=True and dosage=True exclude each other (the EM r is its own estimate from the genotypes)")
    if path not in (None, "fp4"):
        raise _lib.LdxError(f"{what}: em=True runs on the FP4 band only (path must be None or 'fp4', got {path!r})")
    if panel.n_hap % 2:
        raise _lib.LdxError(f"{what}: the EM needs an even n_hap (got {panel.n_hap}): individual k owns haplotypes 2k and 2k + 1")
    return pairwise


def _em_panel(panel: PackedPanel, pairwise: bool) -> tuple:
    """The panel's arguments of the EM band entries: alt, ref, acnt, rcnt (ref and rcnt None unless ``pairwise``)."""
    if pairwise:
        return panel.alt.data_ptr(), panel.ref.data_ptr(), panel.acnt.data_ptr(), panel.rcnt.data_ptr()
    return panel.alt.data_ptr(), None, panel.acnt.data_ptr(), None


def em_snp_stats(panel: PackedPanel, pairwise: bool = False):
    """``(N int32 [n], A int32 [n], diag float32 [n], live uint8 [n])`` on the device (include/ldx.h, ldx_em_snp_stats_dev):
    per SNP the individuals called at it and the sum of their dosages (``pairwise`` False: n_hap / 2 and the ALT count),
    live = 0 < A < 2 N, diag = +1.0 where live, else -0.0: the diagonal of an EM band.  An all-heterozygous SNP is live."""
    if panel.n_hap % 2:
        raise _lib.LdxError(f"em_snp_stats: the EM needs an even n_hap (got {panel.n_hap}): individual k owns haplotypes 2k and "
                            "2k + 1")
    require_gpu()
    n, dev = panel.n_snps, panel.device
    n_called = torch.empty(n, dtype=torch.int32, device=dev)
    a_sum = torch.empty(n, dtype=torch.int32, device=dev)
    diag = torch.empty(n, dtype=torch.float32, device=dev)
    live = torch.empty(n, dtype=torch.uint8, device=dev)
    check(lib.ldx_em_snp_stats_dev(*_em_panel(panel, pairwise), n, panel.n_hap, int(bool(pairwise)), n_called.data_ptr(),
                                   a_sum.data_ptr(), diag.data_ptr(), live.data_ptr(), _stream_ptr()), "ldx_em_snp_stats_dev")
    return n_called, a_sum, diag, live


@dataclass
class LDEmBand:
    """ld_em_band's two bands (None where only the other was asked for): ``r`` and ``dprime`` are LDBands with ``em`` set that
    share the layout tensors and the diagonal -- +1.0 where the SNP has both alleles among its called individuals, else -0.0
    -- so everything an LDBand offers works on ``.r`` as it is.  ``live``: uint8 [n] on the device, the diagonal's rule."""

    r: Optional[LDBand]
    dprime: Optional[LDBand]
    live: torch.Tensor

    @property
    def n_cells(self) -> int:
        return (self.r if self.r is not None else self.dprime).n_cells


def ld_em_band(panel: PackedPanel, positions=None, window_bp: int = 1_000_000, window_snps: Optional[int] = None,
               want_r: bool = True, want_dprime: bool = True, missing: Optional[str] = None,
               workspace: Optional[torch.Tensor] = None, check_positions: bool = True) -> LDEmBand:
    """The windowed EM LD of one panel, kept: for every pair i > j with pos_i - pos_j <= window the r and D' cells of
    ld_em(panel, panel, missing=missing) at (i, j), bit for bit, in ld_band's layout -- what PLINK --r2 dprime --ld-window-kb
    computes, at the cost of the band instead of the square (include/ldx.h, "EM on the band"; ldx_ld_em_band_dev).  Positions
    and window as for ld_band; an even n_hap.  ``want_r`` / ``want_dprime`` = False leaves that band out (None in the result);
    not both.  ``missing``: None (a missing code counts as REF) or "pairwise" (every pair over the individuals called at both
    SNPs); a panel without missing codes gives the same bytes either way.  ``workspace``: a uint8 device tensor of
    ldx_ld_em_band_workspace_bytes() bytes to reuse.  The layout's total is read back once to size the values."""
    pairwise = _em_args("ld_em_band", panel, missing)
    if not (want_r or want_dprime):
        raise _lib.LdxError("ld_em_band: neither r nor D' was asked for")
    require_gpu()
    n, dev = panel.n_snps, panel.device
    pos, pos_h, window = _band_positions(panel, positions, window_bp, window_snps, check_positions, "ld_em_band")
    window = min(window, BAND_WINDOW_MAX)
    workspace = _plan_workspace(lib.ldx_ld_em_band_workspace_bytes, panel, workspace)
    lo, offsets, n_cells = _band_layout(pos, n, window, dev)
    vals = [torch.empty(n_cells, dtype=torch.float32, device=dev) if want else None for want in (want_r, want_dprime)]
    check(lib.ldx_ld_em_band_dev(*_em_panel(panel, pairwise), n, panel.n_hap, int(pairwise), pos.data_ptr(), window, lo.data_ptr(),
                                 offsets.data_ptr(), *(_ptr(v) if v is not None and n_cells else None for v in vals), n_cells,
                                 *_ws(workspace), _stream_ptr()), "ldx_ld_em_band_dev")
    _, _, diag, live = em_snp_stats(panel, pairwise)
    bands = []
    for v in vals:
        band = None
        if v is not None:
            band = LDBand(v, lo, offsets, diag, pos if pos_h is None else pos_h, window, False, panel.n_hap, missing=missing, em=True)
            band._keep = (pos, workspace)   # alive until the launch is done
        bands.append(band)
    return LDEmBand(bands[0], bands[1], live)


def _em_neighbors(panel: PackedPanel, positions, window_bp, window_snps, r2, strict, path, hit_capacity, workspace,
                  check_positions, dosage, missing) -> "LDNeighbors":
    """ld_neighbors(em=True): the pairwise path's buffers and retries around ldx_ld_em_neighbors_dev."""
    pairwise = _em_args("ld_neighbors", panel, missing, path, dosage)
    require_gpu()
    n = panel.n_snps
    bound = r2_bound(r2, strict)
    pos, _, window = _band_positions(panel, positions, window_bp, window_snps, check_positions, "ld_neighbors")
    offsets, hits = _plan_neighbors("ldx_ld_em_neighbors_dev", lib.ldx_ld_em_band_workspace_bytes, panel,
                                    (*_em_panel(panel, pairwise), n, panel.n_hap, int(pairwise)), pos, window, bound, hit_capacity,
                                    workspace)
    return LDNeighbors(offsets, hits, n, window, bound, False, missing, em=True)


EM_PAIRWISE_COUNTS = ("N", "A", "B", "S", "H")   # the order of include/ldx.h, "pairwise-complete EM"


def ld_em_counts(panel_i: PackedPanel, panel_j: Optional[PackedPanel] = None, missing: Optional[str] = None):
    """The two pair counts the EM starts from, as the kernel's K loop produced them: (S, H), int32 [n_i, n_j] each on the
    device -- S = sum_k g_ik g_jk, H = the number of individuals heterozygous at both SNPs (ldx_ld_em_counts_dev).

    ``missing="pairwise"``: the five integers of ld_em(missing="pairwise") over the individuals called at both SNPs, before
    any float: one int32 [5, n_i, n_j] device tensor in the order N A B S H (ldx_ld_em_pw_counts_dev)."""
    pairwise = _rect_missing("ld_em_counts", missing)
    pj = _rect_panels("ld_em_counts", panel_i, panel_j, True)
    require_gpu()
    n_i, n_j, dev = panel_i.n_snps, pj.n_snps, panel_i.device
    if pairwise:
        out = torch.empty((len(EM_PAIRWISE_COUNTS), n_i, n_j), dtype=torch.int32, device=dev)
        check(lib.ldx_ld_em_pw_counts_dev(*_pw_side(panel_i), *_pw_side(pj), panel_i.n_hap, out.data_ptr(), n_j, _stream_ptr()),
              "ldx_ld_em_pw_counts_dev")
        return out
    S = torch.empty((n_i, n_j), dtype=torch.int32, device=dev)
    H = torch.empty((n_i, n_j), dtype=torch.int32, device=dev)
    check(lib.ldx_ld_em_counts_dev(panel_i.alt.data_ptr(), n_i, pj.alt.data_ptr(), n_j, panel_i.n_hap, S.data_ptr(),
                                   H.data_ptr(), n_j, _stream_ptr()), "ldx_ld_em_counts_dev")
    return S, H


def ld_em_from_counts(n_ind, a_i, a_j, S, H, device: Optional[torch.device] = None):
    """The EM epilogue alone on a list of count tuples of ``n_ind`` individuals -- the device function of ld_em's kernels
    (ldx_ld_em_from_counts_dev).  Returns (r float32, dprime float32, x float64) device tensors [m]; a tuple that is no
    genotype table gives NaN in all three.  ``n_ind`` may be an array, one N per tuple -- the pairwise-complete form, whose N
    is the pair's own (ldx_ld_em_from_counts_pw_dev): N = 0 with every other integer 0 is a degenerate pair (-0.0f)."""
    require_gpu()
    dev = device or torch.device("cuda", torch.cuda.current_device())
    per_tuple = hasattr(n_ind, "cpu") or np.ndim(n_ind) > 0
    cols = []
    for name, v in ((("n_ind", n_ind),) if per_tuple else ()) + (("a_i", a_i), ("a_j", a_j), ("S", S), ("H", H)):
        v = np.ascontiguousarray(v.cpu().numpy() if hasattr(v, "cpu") else v).reshape(-1)
        if v.size and (int(v.min()) < 0 or int(v.max()) >= (1 << 32)):
            raise _lib.LdxError(f"ld_em_from_counts: {name} must hold uint32 values")
        cols.append(torch.from_numpy(v.astype(np.int64).astype(np.uint32).view(np.int32)).to(dev))
    m = int(cols[0].numel())
    if any(int(c.numel()) != m for c in cols):
        raise _lib.LdxError("ld_em_from_counts: " + ("n_ind, " if per_tuple else "") + "a_i, a_j, S and H differ in length")
    r = torch.empty(m, dtype=torch.float32, device=dev)
    dprime = torch.empty(m, dtype=torch.float32, device=dev)
    x = torch.empty(m, dtype=torch.float64, device=dev)
    if per_tuple:
        check(lib.ldx_ld_em_from_counts_pw_dev(m, *(c.data_ptr() for c in cols), r.data_ptr(), dprime.data_ptr(), x.data_ptr(),
                                               _stream_ptr()), "ldx_ld_em_from_counts_pw_dev")
        return r, dprime, x
    check(lib.ldx_ld_em_from_counts_dev(int(n_ind), m, cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(),
                                        cols[3].data_ptr(), r.data_ptr(), dprime.data_ptr(), x.data_ptr(), _stream_ptr()),
          "ldx_ld_em_from_counts_dev")
    return r, dprime, x


def _em_root_host(g, dg, lo, hi, glo, ghi):
    """em_root of ldx_em_tile.h: Newton steps kept inside [lo, hi] (g(lo) <= 0 <= g(hi)), bisection otherwise."""
    if glo == 0.0:
        return lo
    if ghi == 0.0:
        return hi
    x = 0.5 * (lo + hi)
    dxold = dx = hi - lo
    gx, dgx = g(x), dg(x)
    for _ in range(128):
        if gx == 0.0:
            break
        if gx < 0.0:
            lo = x
        else:
            hi = x
        bisect = ((x - hi) * dgx - gx) * ((x - lo) * dgx - gx) > 0.0 or abs(2.0 * gx) > abs(dxold * dgx)
        dxold = dx
        if bisect:
            dx = 0.5 * (hi - lo)
            xn = lo + dx
        else:
            dx = gx / dgx
            xn = x - dx
        if xn == x:
            break
        x = xn
        gx, dgx = g(x), dg(x)
    return x


def em_host(n_ind: int, a_i: int, a_j: int, S: int, H: int) -> Tuple[float, float, float]:
    """The kernel's epilogue restated in Python floats (fp64): (x*, r, D') of one count tuple (include/ldx.h, "unphased LD
    by EM"; ldx_em_tile.h, em_cell).  The integers are per pair: with the pair's own (N, A, B, S, H) over the individuals
    called at both SNPs this is the pairwise-complete cell (N = 0 is a degenerate pair).  Documentation and a CPU reference: it follows the device path for path -- H = 0 closed
    form; g monotone or one rising branch with a sign change: one bracketed Newton root, no logarithm; two candidates: the
    larger l, the smaller x on a tie -- but is not promised to match it bit for bit.  A degenerate pair gives (0, -0.0, -0.0),
    a tuple that is no genotype table three NaNs."""
    N, ai, aj, S, H = int(n_ind), int(a_i), int(a_j), int(S), int(H)
    T = 2 * N
    n1 = (S - H) // 2
    n2, n3, n4 = ai - n1 - H, aj - n1 - H, T - ai - aj + n1
    if ai > T or aj > T or H > N or S < H or (S - H) % 2 or min(ai, aj, S, H, n2, n3, n4) < 0:
        return math.nan, math.nan, math.nan
    if ai in (0, T) or aj in (0, T):
        return 0.0, -0.0, -0.0
    x = 0.0
    if H > 0:
        f1, f4, m2, m3, Hf = float(n1), float(n4), float(n2 + H), float(n3 + H), float(H)

        def g(x):
            return x * ((m2 - x) * (m3 - x)) - (Hf - x) * ((f1 + x) * (f4 + x))

        def dg(x):
            h1, h4, h2, h3 = f1 + x, f4 + x, m2 - x, m3 - x
            return (h2 * h3 - x * (h2 + h3)) + (h1 * h4 - (Hf - x) * (h1 + h4))

        def loglik(x):
            h1, h4, h2, h3 = f1 + x, f4 + x, m2 - x, m3 - x
            l14 = (n1 * math.log(h1) if n1 else 0.0) + (n4 * math.log(h4) if n4 else 0.0)
            l23 = (n2 * math.log(h2) if n2 else 0.0) + (n3 * math.log(h3) if n3 else 0.0)
            return (l14 + l23) + Hf * math.log(h1 * h4 + h2 * h3)

        g0, gH = -float(H * n1 * n4), float(H * n2 * n3)
        c2 = n1 + n4 - n2 - n3 - 3 * H
        c1 = (n2 + H) * (n3 + H) - H * (n1 + n4) + n1 * n4
        disc = c2 * c2 - 6 * c1
        if disc <= 0:
            x = _em_root_host(g, dg, 0.0, Hf, g0, gH)
        else:
            sq = math.sqrt(float(disc))
            xa, xb = (-c2 - sq) / 6.0, (-c2 + sq) / 6.0
            have1 = have2 = False
            if xa > 0.0:
                hi1 = min(xa, Hf)
                ghi1 = g(hi1) if xa < Hf else gH
                have1 = ghi1 >= 0.0
            if xb < Hf:
                lo2 = max(xb, 0.0)
                glo2 = g(lo2) if xb > 0.0 else g0
                have2 = glo2 <= 0.0
            if have1 and have2:
                x1, x2 = _em_root_host(g, dg, 0.0, hi1, g0, ghi1), _em_root_host(g, dg, lo2, Hf, glo2, gH)
                x = x2 if loglik(x2) > loglik(x1) else x1
            elif have1:
                x = _em_root_host(g, dg, 0.0, hi1, g0, ghi1)
            elif have2:
                x = _em_root_host(g, dg, lo2, Hf, glo2, gH)
            else:
                x = _em_root_host(g, dg, 0.0, Hf, g0, gH)
    dn = float(T) * x + float(T * n1 - ai * aj)
    r = dn / math.sqrt(float(ai * (T - ai)) * float(aj * (T - aj)))
    dmax = min(ai * (T - aj), (T - ai) * aj) if dn >= 0.0 else min(ai * aj, (T - ai) * (T - aj))
    return x, r, abs(dn) / float(dmax)


# ---- Gabriel blocks: D' confidence bounds on the EM band (include/ldx.h, "Gabriel blocks")
NO_BLOCK = 0xFFFFFFFE            # block_of of a kept SNP that lies in no block (ldx_gabriel_pick_dev)
NO_CI = 0xFF                     # both bounds of a pair without an interval
CI_TAIL = 0.05
GABRIEL_DEFAULTS = dict(cand_cut=70, strong_hi=98, recomb_hi=90, cuts=(80, 50, 50, 70), max_spans=(20_000, 30_000, None, None),
                        min_informative=(1, 3, 6, 6), strong_share=(19, 20))


def gabriel_params(**kw) -> dict:
    """The section-3 parameters with their defaults (GABRIEL_DEFAULTS), checked: cuts / max_spans / min_informative have one
    entry per row m = 2, 3, 4, >= 5 (a max span of None is the window); strong_share = (19, 20) means more than 95 %."""
    unknown = set(kw) - set(GABRIEL_DEFAULTS)
    if unknown:
        raise _lib.LdxError(f"unknown Gabriel parameter(s): {sorted(unknown)}")
    p = {k: kw[k] if kw.get(k) is not None else v for k, v in GABRIEL_DEFAULTS.items()}
    for k in ("cuts", "max_spans", "min_informative"):
        p[k] = tuple(p[k])
        if len(p[k]) != 4:
            raise _lib.LdxError(f"{k} needs four entries (m = 2, 3, 4, >= 5)")
    p["max_spans"] = tuple(-1 if s is None or int(s) < 0 else int(s) for s in p["max_spans"])
    num, den = (int(v) for v in p["strong_share"])
    if den <= 0 or not 0 <= num <= den:
        raise _lib.LdxError("strong_share must be (num, den) with 0 <= num <= den, den > 0")
    p["strong_share"] = (num, den)
    for k in ("cand_cut", "strong_hi", "recomb_hi"):
        p[k] = int(p[k])
    for v in (p["cand_cut"], p["strong_hi"], p["recomb_hi"], *p["cuts"], *p["min_informative"]):
        if not 0 <= int(v) < (1 << 32):
            raise _lib.LdxError("Gabriel parameters must be non-negative 32-bit integers")
    return p


def _gabriel_struct(p: dict) -> "_lib.GabrielParams":
    s = _lib.GabrielParams()
    s.cand_cut, s.strong_hi, s.recomb_hi = p["cand_cut"], p["strong_hi"], p["recomb_hi"]
    for k in range(4):
        s.cut[k], s.max_span[k], s.min_informative[k] = int(p["cuts"][k]), p["max_spans"][k], int(p["min_informative"][k])
    s.frac_num, s.frac_den = p["strong_share"]
    return s


def dprime_ci_host(n_ind, a_i, a_j, S, H):
    """Host mirror (numpy, fp64) of ci_cell (ldx_em_tile.h): the D' confidence bounds (lo, hi) in percent of a count tuple,
    (NO_CI, NO_CI) for a tuple that is no genotype table or a degenerate pair.  Scalars give two ints, arrays (``n_ind`` may
    stay a scalar) two uint8 arrays.  The sign is em_host's r as a float32 cell; a reference, not promised to match the
    device where a cumulative sum grazes the 5 % line."""
    scalar = np.ndim(a_i) == 0
    A, B, S, H = (np.atleast_1d(np.asarray(v, dtype=np.int64)).reshape(-1) for v in (a_i, a_j, S, H))
    N = np.broadcast_to(np.asarray(n_ind, dtype=np.int64).reshape(-1), A.shape)
    m = A.shape[0]
    T = 2 * N
    neg = np.zeros(m, dtype=bool)
    ok = np.zeros(m, dtype=bool)
    for k in range(m):
        r = em_host(int(N[k]), int(A[k]), int(B[k]), int(S[k]), int(H[k]))[1]
        ok[k] = r == r and 0 < A[k] < T[k] and 0 < B[k] < T[k]
        neg[k] = ok[k] and bool(np.float32(r) < 0)
    lo = np.full(m, NO_CI, dtype=np.uint8)
    hi = np.full(m, NO_CI, dtype=np.uint8)
    if ok.any():
        N, T, A, B, S, H, neg_ = N[ok], T[ok], A[ok], B[ok], S[ok], H[ok], neg[ok]
        n1 = (S - H) // 2
        n2, n3, n4 = A - n1 - H, B - n1 - H, T - A - B + n1
        dm = np.where(neg_, np.minimum(A * B, (T - A) * (T - B)), np.minimum(A * (T - B), (T - A) * B))
        step = (np.arange(101, dtype=np.int64)[None, :] * dm[:, None]).astype(np.float64) / 100.0
        base = (A * B).astype(np.float64)[:, None]
        h1 = np.where(neg_[:, None], base - step, base + step) / T.astype(np.float64)[:, None]
        h2 = A.astype(np.float64)[:, None] - h1
        h3 = B.astype(np.float64)[:, None] - h1
        h4 = (T - A - B).astype(np.float64)[:, None] + h1
        h1, h2, h3, h4 = (np.maximum(h, 2.0 ** -20) for h in (h1, h2, h3, h4))

        def term(cnt, h):
            return np.where(cnt[:, None] > 0, cnt.astype(np.float64)[:, None] * np.log(h), 0.0)

        ell = ((term(n1, h1) + term(n4, h4)) + (term(n2, h2) + term(n3, h3))) + term(H, h1 * h4 + h2 * h3)
        w = np.exp(ell - ell.max(axis=1, keepdims=True))
        up = np.cumsum(w, axis=1)                     # ascending sums; W is the last
        down = np.cumsum(w[:, ::-1], axis=1)          # descending sums, from k = 100
        tail = CI_TAIL * up[:, -1:]
        klo = np.argmax(up > tail, axis=1)
        khi = 100 - np.argmax(down > tail, axis=1)
        lo[ok] = np.maximum(klo - 1, 0).astype(np.uint8)
        hi[ok] = np.minimum(khi + 1, 100).astype(np.uint8)
    return (int(lo[0]), int(hi[0])) if scalar else (lo, hi)


def gabriel_kept_host(n_called, a_sum, keep=None, maf_min: float = 0.05) -> np.ndarray:
    """bool [n]: keep & live & (MAF over the SNP's own called individuals >= maf_min), from em_snp_stats' N and A: live iff
    0 < A < 2 N, MAF = min(A, 2 N - A) / (2 N), compared as min(A, 2 N - A) >= maf_min * 2 N in fp64."""
    t = 2 * np.asarray(n_called, dtype=np.int64)
    a = np.asarray(a_sum, dtype=np.int64)
    kept = (a > 0) & (a < t) & (np.minimum(a, t - a).astype(np.float64) >= float(maf_min) * t.astype(np.float64))
    return kept if keep is None else kept & np.asarray(keep).astype(bool)


def gabriel_candidates_host(lo, hi, positions, kept, window: int, **params) -> np.ndarray:
    """Host mirror of ldx_gabriel_candidates_dev: the VALID candidates as int64 [k, 3] rows (first, last, span), ordered by
    first, then last.  ``lo`` / ``hi``: the two bound bands (uint8 [n_cells]) in the layout of band_layout_host(positions,
    window); ``kept`` bool [n]; ``params``: the section-3 parameters (gabriel_params)."""
    p = gabriel_params(**params)
    lo = np.asarray(lo).astype(np.int64)
    hi = np.asarray(hi).astype(np.int64)
    pos = np.asarray(positions, dtype=np.int64)
    kept = np.asarray(kept).astype(bool)
    n = pos.shape[0]
    band_lo, off = band_layout_host(pos, int(window))
    band_lo = np.asarray(band_lo).astype(np.int64)
    off = np.asarray(off).astype(np.int64)
    has = lo != NO_CI
    strong_hi = has & (hi >= p["strong_hi"])
    recomb = hi < p["recomb_hi"]
    # per-row suffix counts over the kept columns, as the device builds them: S at the cuts of rows 1..3, and R
    suf = np.zeros((4, lo.shape[0]), dtype=np.int64)
    for i in range(n):
        a, b = off[i], off[i + 1]
        if b == a or not kept[i]:
            continue
        kj = kept[band_lo[i]:i]
        preds = [strong_hi[a:b] & (lo[a:b] >= p["cuts"][r]) & kj for r in (1, 2, 3)] + [recomb[a:b] & kj]
        for q, pr in enumerate(preds):
            suf[q, a:b] = np.cumsum(pr[::-1])[::-1]
    out = []
    for f in range(n):
        if not kept[f]:
            continue
        tri = np.zeros(4, dtype=np.int64)
        m = 1
        for l in range(f + 1, n):
            if band_lo[l] > f:
                break
            at = off[l] + f - band_lo[l]
            tri += suf[:, at]
            if not kept[l]:
                continue
            m += 1
            if not (strong_hi[at] and lo[at] >= p["cand_cut"]):
                continue
            row = min(m, 5) - 2
            if row == 0:
                n_s, n_r = int(strong_hi[at] and lo[at] >= p["cuts"][0]), int(recomb[at])
            else:
                n_s, n_r = int(tri[row - 1]), int(tri[3])
            span = int(pos[l] - pos[f])
            cap = int(window) if p["max_spans"][row] < 0 else p["max_spans"][row]
            if span <= int(window) and span <= cap and n_s + n_r >= p["min_informative"][row] and \
                    p["strong_share"][1] * n_s > p["strong_share"][0] * (n_s + n_r):
                out.append((f, l, span))
    return np.asarray(out, dtype=np.int64).reshape(-1, 3)


def gabriel_pick_host(cands, n: int, kept=None) -> Tuple[np.ndarray, int]:
    """Host mirror of ldx_gabriel_pick_dev: (block_of uint32 [n], n_blocks) from the valid candidates (rows first, last, span):
    by span descending, ties by smaller first, then smaller last, a candidate is accepted iff no SNP of [first, last] lies in
    an accepted block; blocks are numbered in position order.  ``kept`` (bool [n], default all): NOT_KEPT for the others."""
    cands = np.asarray(cands, dtype=np.int64).reshape(-1, 3)
    kept = np.ones(n, dtype=bool) if kept is None else np.asarray(kept).astype(bool)
    used = np.zeros(n, dtype=bool)
    starts = []
    for k in np.lexsort((cands[:, 1], cands[:, 0], -cands[:, 2])):
        f, l = int(cands[k, 0]), int(cands[k, 1])
        if not used[f:l + 1].any():
            used[f:l + 1] = True
            starts.append(f)
    block_of = np.full(n, NOT_KEPT, dtype=np.uint32)
    block_of[kept] = NO_BLOCK
    flag = np.zeros(n, dtype=np.int64)
    flag[starts] = 1
    number = np.cumsum(flag) - 1
    member = used & kept
    block_of[member] = number[member].astype(np.uint32)
    return block_of, len(starts)


def ld_ci_from_counts(n_ind, a_i, a_j, S, H, device: Optional[torch.device] = None):
    """The D' confidence bounds alone on a list of count tuples -- the device function of ld_dprime_ci's kernel
    (ldx_ld_ci_from_counts_dev).  Returns (lo uint8, hi uint8) device tensors [m]; ``n_ind`` a scalar or one N per tuple."""
    require_gpu()
    dev = device or torch.device("cuda", torch.cuda.current_device())
    m = int(np.size(a_i.cpu().numpy() if hasattr(a_i, "cpu") else a_i))
    if not (hasattr(n_ind, "cpu") or np.ndim(n_ind) > 0):
        n_ind = np.full(m, int(n_ind), dtype=np.int64)
    cols = []
    for name, v in (("n_ind", n_ind), ("a_i", a_i), ("a_j", a_j), ("S", S), ("H", H)):
        v = np.ascontiguousarray(v.cpu().numpy() if hasattr(v, "cpu") else v).reshape(-1)
        if v.size and (int(v.min()) < 0 or int(v.max()) >= (1 << 32)):
            raise _lib.LdxError(f"ld_ci_from_counts: {name} must hold uint32 values")
        if v.size != m:
            raise _lib.LdxError("ld_ci_from_counts: n_ind, a_i, a_j, S and H differ in length")
        cols.append(torch.from_numpy(v.astype(np.int64).astype(np.uint32).view(np.int32)).to(dev))
    lo = torch.empty(m, dtype=torch.uint8, device=dev)
    hi = torch.empty(m, dtype=torch.uint8, device=dev)
    if m:
        check(lib.ldx_ld_ci_from_counts_dev(m, *(c.data_ptr() for c in cols), lo.data_ptr(), hi.data_ptr(), _stream_ptr()),
              "ldx_ld_ci_from_counts_dev")
    return lo, hi


@dataclass
class LDCiBand:
    """ld_dprime_ci's two bands: ``lo`` / ``hi`` uint8 [n_cells] on the device, the D' confidence bounds in percent of every
    in-window pair i > j at ``offsets[i] + j - band_lo[i]`` (ld_band's layout); NO_CI in both for a pair without an interval
    or with a SNP that is not kept.  ``kept``: uint8 [n] on the device -- keep & MAF & live."""

    lo: torch.Tensor
    hi: torch.Tensor
    band_lo: torch.Tensor
    offsets: torch.Tensor
    kept: torch.Tensor
    positions: object
    window: int
    n_cells: int
    missing: Optional[str] = None

    @property
    def n_snps(self) -> int:
        return int(self.band_lo.numel())

    def layout(self) -> Tuple[np.ndarray, np.ndarray]:
        """(lo int64 [n], offsets int64 [n + 1]) on the host."""
        return self.band_lo.cpu().numpy().astype(np.int64), self.offsets.cpu().numpy().astype(np.int64)

    def strong(self, cut: int = 70, strong_hi: int = 98) -> torch.Tensor:
        """bool [n_cells] on the device: lo != NO_CI, lo >= cut and hi >= strong_hi."""
        return (self.lo != NO_CI) & (self.lo >= int(cut)) & (self.hi >= int(strong_hi))

    def recombinant(self, recomb_hi: int = 90) -> torch.Tensor:
        """bool [n_cells] on the device: hi < recomb_hi (a pair without an interval never is)."""
        return self.hi < int(recomb_hi)

    def to_dense(self) -> Tuple[np.ndarray, np.ndarray]:
        """(lo, hi) as symmetric uint8 [n, n] host arrays, NO_CI on the diagonal and outside the band."""
        n = self.n_snps
        band_lo, off = self.layout()
        lo_h, hi_h = self.lo.cpu().numpy(), self.hi.cpu().numpy()
        out = [np.full((n, n), NO_CI, dtype=np.uint8) for _ in range(2)]
        rows = np.repeat(np.arange(n), np.diff(off))
        cols = np.arange(off[-1]) - off[rows] + band_lo[rows]
        for d, v in zip(out, (lo_h, hi_h)):
            d[rows, cols] = v
            d[cols, rows] = v
        return out[0], out[1]


def ld_dprime_ci(panel: PackedPanel, positions=None, window_bp: int = 500_000, window_snps: Optional[int] = None,
                 missing: Optional[str] = None, keep=None, maf_min: float = 0.05, workspace: Optional[torch.Tensor] = None,
                 check_positions: bool = True) -> LDCiBand:
    """Gabriel's D' confidence bounds of every in-window pair, on the EM band (include/ldx.h, "Gabriel blocks";
    ldx_ld_em_ci_band_dev): for i > j with pos_i - pos_j <= window, both SNPs kept, the 5 % tails of the likelihood of the
    pair's genotype table over D' = 0 .. 100 % on the side of the EM estimate's sign, as two bytes in ld_band's layout.  A SNP
    is kept iff ``keep`` (bool [n], default all) and its MAF over its own called individuals is >= ``maf_min`` and it has both
    alleles among them; a cell with a SNP not kept holds NO_CI.  Positions, window, ``missing`` and ``workspace`` as for
    ld_em_band.  This project's own definition after Gabriel et al. 2002, not validated against PLINK or Haploview."""
    pairwise = _em_args("ld_dprime_ci", panel, missing)
    if not 0.0 <= float(maf_min) <= 0.5:
        raise _lib.LdxError("maf_min must lie in [0, 0.5]")
    n = panel.n_snps
    kmask = _keep_mask(keep, n)
    require_gpu()
    dev = panel.device
    pos, pos_h, window = _band_positions(panel, positions, window_bp, window_snps, check_positions, "ld_dprime_ci")
    window = min(window, BAND_WINDOW_MAX)
    workspace = _plan_workspace(lib.ldx_ld_em_band_workspace_bytes, panel, workspace)
    n_called, a_sum, _, live = em_snp_stats(panel, pairwise)
    t = 2 * n_called.to(torch.int64)
    a = a_sum.to(torch.int64)
    kept = live.bool() & (torch.minimum(a, t - a).to(torch.float64) >= float(maf_min) * t.to(torch.float64))
    if kmask is not None:
        kept = kept & torch.as_tensor(kmask).to(dev)
    kept = kept.to(torch.uint8).contiguous()
    lo, offsets, n_cells = _band_layout(pos, n, window, dev)
    ci_lo = torch.empty(n_cells, dtype=torch.uint8, device=dev)
    ci_hi = torch.empty(n_cells, dtype=torch.uint8, device=dev)
    check(lib.ldx_ld_em_ci_band_dev(*_em_panel(panel, pairwise), n, panel.n_hap, int(pairwise), pos.data_ptr(), window,
                                    kept.data_ptr(), lo.data_ptr(), offsets.data_ptr(), _ptr(ci_lo) if n_cells else None,
                                    _ptr(ci_hi) if n_cells else None, n_cells, *_ws(workspace), _stream_ptr()),
          "ldx_ld_em_ci_band_dev")
    res = LDCiBand(ci_lo, ci_hi, lo, offsets, kept, pos if pos_h is None else pos_h, window, n_cells, missing)
    res._keep = (pos, workspace)   # alive until the launch is done
    return res


@dataclass
class GabrielBlocks:
    """Haplotype blocks by Gabriel's rule (ld_gabriel_blocks).  ``block_of_dev`` / ``n_out`` are the device tensors the pick
    wrote (int32 views of the uint32 words); the host arrays are fetched when first asked for.  ``ci``: the bounds' band."""

    block_of_dev: torch.Tensor
    n_out: torch.Tensor
    ci: LDCiBand
    params: dict
    _host: Optional[tuple] = None

    def _fetch(self) -> tuple:
        if self._host is None:
            block_of = self.block_of_dev.cpu().numpy().view(np.uint32)
            n_out = self.n_out.cpu().numpy().view(np.uint32)
            pos = self.ci.positions
            pos = np.asarray(pos.cpu().numpy() if isinstance(pos, torch.Tensor) else pos, dtype=np.int64)
            nb = int(n_out[0])
            members = np.flatnonzero(block_of < NO_BLOCK)
            b = block_of[members].astype(np.int64)
            starts = np.full(nb, -1, dtype=np.int64)
            ends = np.full(nb, -1, dtype=np.int64)
            starts[b[::-1]] = members[::-1]   # the first member wins
            ends[b] = members                 # the last member wins
            self._host = (block_of, nb, int(n_out[1]), starts, ends, np.bincount(b, minlength=nb).astype(np.int64), pos)
        return self._host

    @property
    def block_of(self) -> np.ndarray:
        """uint32 [n]: the 0-based block (in position order) of every member, NO_BLOCK for a kept SNP in no block, NOT_KEPT
        for a SNP that is not kept."""
        return self._fetch()[0]

    @property
    def n_blocks(self) -> int:
        return self._fetch()[1]

    @property
    def n_candidates(self) -> int:
        """The valid candidates the pick went through."""
        return self._fetch()[2]

    @property
    def starts(self) -> np.ndarray:
        """int64 [n_blocks]: the first SNP of every block."""
        return self._fetch()[3]

    @property
    def ends(self) -> np.ndarray:
        """int64 [n_blocks]: the last SNP of every block (inclusive)."""
        return self._fetch()[4]

    @property
    def sizes(self) -> np.ndarray:
        """int64 [n_blocks]: members (kept SNPs) per block."""
        return self._fetch()[5]

    @property
    def spans_bp(self) -> np.ndarray:
        pos = self._fetch()[6]
        return pos[self.ends] - pos[self.starts]


def ld_gabriel_blocks(panel: PackedPanel, positions=None, window_bp: int = 500_000, window_snps: Optional[int] = None,
                      missing: Optional[str] = None, keep=None, maf_min: float = 0.05, workspace: Optional[torch.Tensor] = None,
                      check_positions: bool = True, dosage: bool = False, path: Optional[str] = None, **params) -> GabrielBlocks:
    """Haplotype blocks by Gabriel et al.'s D' confidence-interval rule -- what PLINK --blocks and Haploview pick by default --
    from unphased genotypes (include/ldx.h, "Gabriel blocks"): ld_dprime_ci's bounds, then the candidates (first, last) whose
    end pair is strong and whose inside pairs are more than 95 % strong among the informative ones, then the greedy pick by
    span.  ``params``: cand_cut, strong_hi, recomb_hi, cuts, max_spans, min_informative, strong_share (GABRIEL_DEFAULTS).
    Everything is stream-ordered; beyond the layout's total the host reads nothing until a result property is asked for.
    ``dosage=True`` and a haplotype ``path`` are refused, as the EM operators refuse them."""
    _em_args("ld_gabriel_blocks", panel, missing, path, dosage)
    p = gabriel_params(**params)
    ci = ld_dprime_ci(panel, positions, window_bp, window_snps, missing, keep, maf_min, workspace, check_positions)
    n, dev, n_cells = panel.n_snps, panel.device, ci.n_cells
    pos = ci._keep[0]
    span = torch.empty(n_cells, dtype=torch.int64, device=dev)
    first = torch.empty(n_cells, dtype=torch.int32, device=dev)
    last = torch.empty(n_cells, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.ldx_gabriel_candidates_workspace_bytes(n, n_cells) + lib.ldx_gabriel_pick_workspace_bytes(n),
                     dtype=torch.uint8, device=dev)
    pick_ws = ws[lib.ldx_gabriel_candidates_workspace_bytes(n, n_cells):]
    prm = _gabriel_struct(p)
    nz = bool(n_cells)
    check(lib.ldx_gabriel_candidates_dev(_ptr(ci.lo) if nz else None, _ptr(ci.hi) if nz else None, ci.band_lo.data_ptr(),
                                         ci.offsets.data_ptr(), n_cells, pos.data_ptr(), ci.kept.data_ptr(), n, ci.window,
                                         ctypes.addressof(prm), _ptr(span) if nz else None, _ptr(first) if nz else None,
                                         _ptr(last) if nz else None, ws.data_ptr(), ws.numel(), _stream_ptr()),
          "ldx_gabriel_candidates_dev")
    sorted_span, order = torch.sort(span, descending=True, stable=True)
    block_of = torch.empty(n, dtype=torch.int32, device=dev)
    n_out = torch.empty(2, dtype=torch.int32, device=dev)
    check(lib.ldx_gabriel_pick_dev(_ptr(sorted_span) if nz else None, _ptr(order) if nz else None, _ptr(first) if nz else None,
                                   _ptr(last) if nz else None, n_cells, ci.kept.data_ptr(), n, block_of.data_ptr(),
                                   n_out.data_ptr(), pick_ws.data_ptr(), pick_ws.numel(), _stream_ptr()), "ldx_gabriel_pick_dev")
    res = GabrielBlocks(block_of, n_out, ci, p)
    res._keep = (ws, sorted_span, order, first, last, span)   # alive until the launches are done
    return res


# --------------------------------------------------------------------------- sample relatedness (individual x individual)
SAMPLE_COUNTS = ("N", "HH", "IBS0", "HET")     # the planes of ldx_sample_counts_dev, in its order
SAMPLE_STORE_SNPS = 1 << 18                    # SNPs per transposed store of sample_counts: 96 KiB per individual


def _u32_to_i64(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def float32_bound(t: float, strict: bool = False) -> np.float32:
    """The float32 b with ``x >= b`` equal to ``x >= t`` (``x > t`` when strict) for every float32 x: the smallest float32 not
    below (strict: above) t."""
    t = float(t)
    if np.isnan(t):
        raise _lib.LdxError("the bound must not be NaN")
    with np.errstate(over="ignore"):
        b = np.float32(t)
    if float(b) < t or (strict and float(b) == t):
        b = np.nextafter(b, np.float32(np.inf), dtype=np.float32)
    return np.float32(b)


@dataclass
class RelatedPairs:
    """The pairs a > b of SampleCounts.related, as numpy arrays of one length: the two individuals, the kinship cell and the
    pair's counts."""

    a: np.ndarray
    b: np.ndarray
    kin: np.ndarray
    n: np.ndarray
    hethet: np.ndarray
    ibs0: np.ndarray

    def __len__(self) -> int:
        return int(self.a.size)


@dataclass
class SampleCounts:
    """The integer co-occurrence counts between the individuals of a panel over its kept SNPs (include/ldx.h, "sample
    relatedness"): ``counts`` int32 [4, n_ind, n_ind] on the device (uint32 bit patterns, planes N, HH, IBS0, HET), and
    ``n_snps``, the SNPs walked so far (kept or not) by the calls that accumulated into it."""

    counts: torch.Tensor
    n_snps: int

    @property
    def n_ind(self) -> int:
        return int(self.counts.shape[1])

    @property
    def n(self) -> torch.Tensor:
        """uint32 [n_ind, n_ind]: SNPs called in both."""
        return self.counts[0].view(torch.uint32)

    @property
    def hethet(self) -> torch.Tensor:
        """uint32 [n_ind, n_ind]: SNPs heterozygous in both."""
        return self.counts[1].view(torch.uint32)

    @property
    def ibs0(self) -> torch.Tensor:
        """uint32 [n_ind, n_ind]: opposite homozygotes."""
        return self.counts[2].view(torch.uint32)

    @property
    def het(self) -> torch.Tensor:
        """uint32 [n_ind, n_ind]: het[a, b] = SNPs where a is heterozygous and b called (het[b, a] is the partner's)."""
        return self.counts[3].view(torch.uint32)

    @property
    def ibs1(self) -> torch.Tensor:
        """int64 [n_ind, n_ind]: HET[a][b] + HET[b][a] - 2 HH."""
        het = _u32_to_i64(self.counts[3])
        return het + het.T - 2 * _u32_to_i64(self.counts[1])

    @property
    def ibs2(self) -> torch.Tensor:
        """int64 [n_ind, n_ind]: N - IBS1 - IBS0."""
        return _u32_to_i64(self.counts[0]) - self.ibs1 - _u32_to_i64(self.counts[2])

    def _cells(self, want_kin: bool, want_ibs: bool):
        n = self.n_ind
        dev = self.counts.device
        kin = torch.empty((n, n), dtype=torch.float32, device=dev) if want_kin else None
        ibs = torch.empty((n, n), dtype=torch.float32, device=dev) if want_ibs else None
        check(lib.ldx_sample_cells_dev(self.counts.data_ptr(), n, n, _ptr(kin), _ptr(ibs), n, _stream_ptr()), "ldx_sample_cells_dev")
        return kin, ibs

    def kinship(self) -> torch.Tensor:
        """float32 [n_ind, n_ind] on the device: the KING-robust kinship cell of every pair (-0.0f where the smaller HET is 0)."""
        return self._cells(True, False)[0]

    def ibs(self) -> torch.Tensor:
        """float32 [n_ind, n_ind] on the device: the IBS similarity (2 IBS2 + IBS1) / (2 N) (-0.0f where N is 0)."""
        return self._cells(False, True)[1]

    def related(self, kin_min: float, strict: bool = False) -> RelatedPairs:
        """The pairs a > b whose kinship cell is >= kin_min (strict: > kin_min), a float32 comparison, in row-major order."""
        kin = self.kinship()
        bound = torch.tensor(float(float32_bound(kin_min, strict)), dtype=torch.float32, device=kin.device)
        lower = torch.ones_like(kin, dtype=torch.bool).tril(-1)
        idx = torch.nonzero((kin >= bound) & lower)
        a, b = idx[:, 0], idx[:, 1]
        take = lambda k: _u32_to_i64(self.counts[k][a, b]).cpu().numpy()  # noqa: E731
        return RelatedPairs(a.cpu().numpy(), b.cpu().numpy(), kin[a, b].cpu().numpy(), take(0), take(1), take(2))


def _store_args(what: str, panel: PackedPanel, keep, store_snps) -> Tuple[int, Optional[torch.Tensor]]:
    """The argument rules of the operators that build individual-major stores (sample_counts, GenoOperator), checked before
    anything touches the device: an even n_hap, ``store_snps`` within the library's range, a boolean ``keep``.  Returns
    (store_snps, the keep mask on the device or None)."""
    _even_n_hap(what, panel)
    store_snps = int(store_snps)
    if not (1 <= store_snps <= _lib.KING_MAX_STORE_SNPS):
        raise _lib.LdxError(f"{what}: store_snps must lie in 1..{_lib.KING_MAX_STORE_SNPS}")
    return store_snps, _keep_dev(keep, panel.n_snps, panel.device)


def _planes_launch(panel: PackedPanel, keep_d, begin: int, count: int, store, tables) -> None:
    """Transpose the SNPs [begin, begin + count) of the panel into one individual-major store and its tables."""
    check(lib.ldx_sample_planes_dev(panel.alt.data_ptr(), panel.ref.data_ptr(), panel.n_snps, panel.n_hap, _ptr(keep_d), begin,
                                    count, store.data_ptr(), tables.data_ptr(), _stream_ptr()), "ldx_sample_planes_dev")


def sample_counts(panel: PackedPanel, keep=None, out: Optional[SampleCounts] = None, n_slices: Optional[int] = None,
                  store_snps: int = SAMPLE_STORE_SNPS) -> SampleCounts:
    """The counts N, HH, IBS0, HET between the individuals of ``panel`` (haplotypes 2a, 2a + 1 are individual a) over the SNPs
    that pass ``keep`` (a boolean mask [n_snps]; None = all): the panel is transposed on the device into individual-major bit
    planes, ``store_snps`` SNPs at a time (ldx_sample_planes_dev), and counted on the FP4 matrix cores (ldx_sample_counts_dev).
    ``out``: an earlier result of the same individuals to add to -- chromosomes, or chunks of a fileset, sum into one result.
    ``n_slices``: the K slices per tile (None: the library's choice).  Every cell is an exact integer; the result does not
    depend on the order or the split of the SNPs."""
    require_gpu()
    store_snps, keep_d = _store_args("sample_counts", panel, keep, store_snps)
    n_ind, n_snps, dev = panel.n_ind, panel.n_snps, panel.device
    if out is None:
        res = SampleCounts(torch.empty((len(SAMPLE_COUNTS), n_ind, n_ind), dtype=torch.int32, device=dev), 0)
        accumulate = 0
    else:
        if out.n_ind != n_ind or out.counts.device != dev:
            raise _lib.LdxError(f"sample_counts: out holds {out.n_ind} individuals on {out.counts.device}, the panel {n_ind} on {dev}")
        res, accumulate = out, 1
    width = min(store_snps, n_snps)
    store = torch.empty(lib.ldx_sample_planes_bytes(n_ind, width), dtype=torch.uint8, device=dev)
    tables = torch.empty(lib.ldx_sample_tables_bytes(n_ind) // 4, dtype=torch.int32, device=dev)
    for begin in range(0, n_snps, store_snps):
        count = min(store_snps, n_snps - begin)
        _planes_launch(panel, keep_d, begin, count, store, tables)
        check(lib.ldx_sample_counts_dev(store.data_ptr(), tables.data_ptr(), n_ind, count, res.counts.data_ptr(), n_ind, accumulate,
                                        res.n_snps if accumulate else 0, int(n_slices or 0), _stream_ptr()), "ldx_sample_counts_dev")
        res.n_snps += count
        accumulate = 1
    res._keep = (store, tables, keep_d)   # alive until the launches are done
    return res


def king_kinship(panel: PackedPanel, keep=None) -> torch.Tensor:
    """float32 [n_ind, n_ind] on the device: ``sample_counts(panel, keep).kinship()``."""
    return sample_counts(panel, keep).kinship()


def ibs_matrix(panel: PackedPanel, keep=None) -> torch.Tensor:
    """float32 [n_ind, n_ind] on the device: ``sample_counts(panel, keep).ibs()``."""
    return sample_counts(panel, keep).ibs()


def sample_counts_host(codes, keep=None) -> np.ndarray:
    """Host mirror of sample_counts in pure numpy: int64 [4, n_ind, n_ind] (N, HH, IBS0, HET) from the allele codes [n_snps,
    n_hap] (1 = ALT, 0 = REF, anything else = missing).  float64 GEMMs of 0/1 matrices: exact below 2^53."""
    c = np.asarray(codes)
    if c.ndim != 2 or c.shape[1] % 2 or c.shape[1] == 0:
        raise _lib.LdxError(f"sample_counts_host: codes [n_snps, n_hap] with an even n_hap needed, got shape {c.shape}")
    k = _keep_mask(keep, c.shape[0])
    if k is not None:
        c = c[k]
    h0, h1 = c[:, 0::2], c[:, 1::2]
    called = ((h0 == 0) | (h0 == 1)) & ((h1 == 0) | (h1 == 1))
    g = ((h0 == 1).astype(np.int8) + (h1 == 1).astype(np.int8)) * called
    q = called.T.astype(np.float64)
    t = ((g == 1) & called).T.astype(np.float64)
    z = ((g == 2) & called).T.astype(np.float64)
    r = ((g == 0) & called).T.astype(np.float64)
    sets = [q @ q.T, t @ t.T, r @ z.T + z @ r.T, t @ q.T]
    return np.stack(sets).astype(np.int64)


def _cell_ints(N, HH, IBS0, HETa, HETb):
    N, HH, IBS0, HETa, HETb = (np.asarray(x).astype(np.int64) for x in (N, HH, IBS0, HETa, HETb))
    ibs1 = HETa + HETb - 2 * HH
    return N, IBS0, ibs1, np.minimum(HETa, HETb)


def king_cell_host(N, HH, IBS0, HETa, HETb) -> np.ndarray:
    """Host mirror of the kinship cell (include/ldx.h, "sample relatedness"): float32, -0.0f where min(HETa, HETb) is 0."""
    N, IBS0, ibs1, m = _cell_ints(N, HH, IBS0, HETa, HETb)
    num, den = (4 * IBS0 + ibs1).astype(np.float64), (4 * m).astype(np.float64)
    val = (0.5 - num / np.where(m > 0, den, 1.0)).astype(np.float32)
    return np.where(m > 0, val, np.float32(-0.0)).astype(np.float32)


def ibs_cell_host(N, HH, IBS0, HETa, HETb) -> np.ndarray:
    """Host mirror of the IBS cell: float32 (2 IBS2 + IBS1) / (2 N), -0.0f where N is 0."""
    N, IBS0, ibs1, _ = _cell_ints(N, HH, IBS0, HETa, HETb)
    ibs2 = N - ibs1 - IBS0
    val = ((2 * ibs2 + ibs1).astype(np.float64) / np.where(N > 0, (2 * N).astype(np.float64), 1.0)).astype(np.float32)
    return np.where(N > 0, val, np.float32(-0.0)).astype(np.float32)


def king_from_counts(N, HH, IBS0, HETa, HETb, device: Optional[torch.device] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The two cells alone on a list of count tuples -- the device functions of the dense cells (ldx_king_from_counts_dev).
    Returns (kin, ibs), float32 device tensors [m]."""
    require_gpu()
    dev = device or torch.device("cuda", torch.cuda.current_device())
    cols = []
    for name, v in (("N", N), ("HH", HH), ("IBS0", IBS0), ("HETa", HETa), ("HETb", HETb)):
        v = np.ascontiguousarray(v.cpu().numpy() if hasattr(v, "cpu") else v).reshape(-1)
        if v.size and (int(v.min()) < 0 or int(v.max()) >= (1 << 32)):
            raise _lib.LdxError(f"king_from_counts: {name} must hold uint32 values")
        cols.append(torch.from_numpy(v.astype(np.int64).astype(np.uint32).view(np.int32)).to(dev))
    m = int(cols[0].numel())
    if any(int(c.numel()) != m for c in cols):
        raise _lib.LdxError("king_from_counts: N, HH, IBS0, HETa and HETb differ in length")
    kin = torch.empty(m, dtype=torch.float32, device=dev)
    ibs = torch.empty(m, dtype=torch.float32, device=dev)
    check(lib.ldx_king_from_counts_dev(m, *(c.data_ptr() for c in cols), kin.data_ptr(), ibs.data_ptr(), _stream_ptr()),
          "ldx_king_from_counts_dev")
    return kin, ibs


def king_cutoff(kin, cutoff: float) -> Tuple[np.ndarray, np.ndarray]:
    """A maximal set of individuals no two of which are related above ``cutoff``: edges are the pairs with kin > cutoff (a
    float32 comparison); the individuals are ranked by (number of edges ascending, index ascending) and the kept set is the
    lexicographically first maximal independent set in that rank (select_host on the CSR of the edges).  Returns (keep bool
    [n_ind], removed_because_of int64 [n_ind]: the kept individual that removed this one, -1 for a kept one)."""
    k = kin.cpu().numpy() if isinstance(kin, torch.Tensor) else np.asarray(kin)
    if k.ndim != 2 or k.shape[0] != k.shape[1]:
        raise _lib.LdxError(f"king_cutoff: a square kinship matrix is needed, got shape {k.shape}")
    n = k.shape[0]
    edge = k.astype(np.float32) >= float32_bound(cutoff, strict=True)
    edge = edge | edge.T
    np.fill_diagonal(edge, False)
    degree = edge.sum(axis=1)
    order = np.lexsort((np.arange(n), degree))
    rank = np.empty(n, dtype=np.uint32)
    rank[order] = np.arange(n, dtype=np.uint32)
    rows, nbr = np.nonzero(edge)
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=offsets[1:])
    state, owner = select_host(offsets, nbr, rank, np.ones(n, dtype=np.uint8))
    keep = state == SEL_INDEX
    return keep, np.where(keep, -1, owner).astype(np.int64)


# --------------------------------------------------------------------------- genotype products, sample PCA, polygenic scores
GENO_SCALE_BITS = 30                           # a quantised weight is rint(2^30 x 2^-e): |q| <= 2^30


def _as_f64_2d(x, what: str) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if t.is_complex() or t.dtype == torch.bool:
        raise _lib.LdxError(f"{what} must be real (got {t.dtype})")
    if t.ndim != 2:
        raise _lib.LdxError(f"{what} must have shape [n, k], got {tuple(t.shape)}")
    return t


def geno_quantize(*mats, device=None):
    """Float matrices [n, k] that share column exponents, as the fixed-point weights of the genotype products: e_c is the
    smallest integer with max |x[:, c]| 2^-e_c <= 1 over all matrices given (matvec_rhs's rule; an all-zero column keeps e = 0)
    and q = rint(2^30 x 2^-e) as int32, round-half-even, every step in fp64 (the scaling by a power of two is exact).  Returns
    (list of int32 tensors, e int64 [k]) on ``device`` (default: where the first matrix is; numpy input stays on the host)."""
    if not mats:
        raise _lib.LdxError("geno_quantize: no matrix given")
    ts = [_as_f64_2d(m, "geno_quantize: a matrix") for m in mats]
    dev = torch.device(device) if device is not None else ts[0].device
    ts = [t.to(dev).to(torch.float64) for t in ts]
    n, k = ts[0].shape
    if any(t.shape[1] != k for t in ts):
        raise _lib.LdxError("geno_quantize: the matrices differ in their number of columns")
    if not 1 <= k <= _lib.GENO_MAX_COLS:
        raise _lib.LdxError(f"geno_quantize: 1 to {_lib.GENO_MAX_COLS} columns per call (got {k})")
    big = torch.zeros(k, dtype=torch.float64, device=dev)
    for t in ts:
        if not bool(torch.isfinite(t).all().item()):
            raise _lib.LdxError("geno_quantize: the matrices must be finite")
        if t.shape[0]:
            big = torch.maximum(big, t.abs().amax(dim=0))
    mant, e = torch.frexp(big)                              # big = mant 2^e, mant in [0.5, 1)
    e = e.to(torch.int64) - (mant == 0.5).to(torch.int64)   # the smallest e with big 2^-e <= 1
    e = torch.where(big > 0, e, torch.zeros_like(e)).clamp(-990, 1000)
    scale = _pow2(GENO_SCALE_BITS - e)
    return [torch.round(t * scale).to(torch.int32).contiguous() for t in ts], e


@dataclass
class GenoProduct:
    """A genotype product (GenoOperator): ``sums``, the int64 device tensor the kernel wrote, in units of 2^(e_c - 30), and
    ``exps``, device int64 [k], the columns' exponents."""

    sums: torch.Tensor
    exps: torch.Tensor

    def values(self) -> torch.Tensor:
        """float64 device tensor shaped like ``sums``: sums 2^(e - 30)."""
        return self.sums.to(torch.float64) * _pow2(self.exps - GENO_SCALE_BITS)


def _geno_weights(what: str, q, rows: int, dev, k: Optional[int] = None) -> torch.Tensor:
    t = q if isinstance(q, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(q))
    if t.dtype != torch.int32 or t.ndim != 2 or t.shape[0] != rows or not 1 <= t.shape[1] <= _lib.GENO_MAX_COLS:
        raise _lib.LdxError(f"{what}: int32 weights [{rows}, k], k in 1..{_lib.GENO_MAX_COLS}, needed; got {t.dtype} {tuple(t.shape)}")
    if k is not None and t.shape[1] != k:
        raise _lib.LdxError(f"{what}: {t.shape[1]} columns beside {k}")
    t = t.to(dev).contiguous()
    lo, hi = torch.aminmax(t)
    if int(lo.item()) < -(1 << GENO_SCALE_BITS) or int(hi.item()) > (1 << GENO_SCALE_BITS):
        raise _lib.LdxError(f"{what}: the weights must lie in -2^30 .. 2^30")
    return t


def _rmatmul_launch(panel: PackedPanel, keep_d: Optional[torch.Tensor], u: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The reverse product's launch on checked weights ``u`` (_geno_weights, [n_ind, k]): (z, zc), int64 [n_snps, k] each.  It reads
    the panel's own planes, so a caller that needs no forward product (ld_glm) calls it without a GenoOperator and its stores."""
    k = int(u.shape[1])
    z = torch.empty((panel.n_snps, k), dtype=torch.int64, device=panel.device)
    zc = torch.empty((panel.n_snps, k), dtype=torch.int64, device=panel.device)
    check(lib.ldx_geno_rmatmul_dev(panel.alt.data_ptr(), panel.ref.data_ptr(), panel.n_snps, panel.n_hap, _ptr(keep_d), u.data_ptr(),
                                   k, k, z.data_ptr(), zc.data_ptr(), k, _stream_ptr()), "ldx_geno_rmatmul_dev")
    return z, zc


class GenoOperator:
    """The operator A = [G | C] of a panel over the SNPs that pass ``keep`` (include/ldx.h, "genotype products"): G the ALT
    dosages of the individuals (0 where missing), C the called flags.  The individual-major store(s) of the forward product are
    built once here, ``store_snps`` SNPs each (ldx_sample_planes_dev), and kept, so that an iteration does not transpose the
    panel again; the reverse product reads the panel's own planes.  All sums are exact integers."""

    def __init__(self, panel: PackedPanel, keep=None, store_snps: int = SAMPLE_STORE_SNPS):
        require_gpu()
        store_snps, self._keep_d = _store_args("GenoOperator", panel, keep, store_snps)
        self.panel, self.n_ind, self.n_snps, self.device = panel, panel.n_ind, panel.n_snps, panel.device
        self._stores = []
        for begin in range(0, self.n_snps, store_snps):
            count = min(store_snps, self.n_snps - begin)
            store = torch.empty(lib.ldx_sample_planes_bytes(self.n_ind, count), dtype=torch.uint8, device=self.device)
            tables = torch.empty(lib.ldx_sample_tables_bytes(self.n_ind) // 4, dtype=torch.int32, device=self.device)
            _planes_launch(panel, self._keep_d, begin, count, store, tables)
            self._stores.append((begin, count, store, tables))

    def called_counts(self) -> torch.Tensor:
        """int64 device tensor [n_ind]: the kept SNPs at which each individual is called (the stores' tables)."""
        total = torch.zeros(self.n_ind, dtype=torch.int64, device=self.device)
        for _, _, _, tables in self._stores:
            total += _u32_to_i64(tables[:self.n_ind])
        return total

    def matmul_q(self, q_w, q_wc=None, n_slices: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """y = G q_w + C q_wc on raw int32 weights [n_snps, k]: int64 device tensor [n_ind, k].  ``out``: an earlier result to
        add to.  ``n_slices``: the K slices per store (None: the library's choice)."""
        w = _geno_weights("matmul_q", q_w, self.n_snps, self.device)
        k = int(w.shape[1])
        wc = None if q_wc is None else _geno_weights("matmul_q", q_wc, self.n_snps, self.device, k)
        if out is None:
            y, accumulate = torch.empty((self.n_ind, k), dtype=torch.int64, device=self.device), 0
        else:
            if out.dtype != torch.int64 or tuple(out.shape) != (self.n_ind, k) or not out.is_contiguous() or out.device != self.device:
                raise _lib.LdxError(f"matmul_q: out must be a contiguous int64 [{self.n_ind}, {k}] tensor on {self.device}")
            y, accumulate = out, 1
        for begin, count, store, tables in self._stores:
            off = begin * k * 4
            check(lib.ldx_geno_matmul_dev(store.data_ptr(), tables.data_ptr(), self.n_ind, count, w.data_ptr() + off,
                                          None if wc is None else wc.data_ptr() + off, k, k, y.data_ptr(), k, accumulate,
                                          int(n_slices or 0), _stream_ptr()), "ldx_geno_matmul_dev")
            accumulate = 1
        return y

    def rmatmul_q(self, q_u) -> Tuple[torch.Tensor, torch.Tensor]:
        """(z, zc) = (G^T q_u, C^T q_u) on raw int32 weights [n_ind, k]: two int64 device tensors [n_snps, k]; the rows of SNPs
        that are not kept are 0."""
        return _rmatmul_launch(self.panel, self._keep_d, _geno_weights("rmatmul_q", q_u, self.n_ind, self.device))

    def matmul(self, W, Wc=None, n_slices: Optional[int] = None) -> GenoProduct:
        """G W + C Wc for float matrices [n_snps, k] (geno_quantize: they share the column exponents)."""
        qs, e = geno_quantize(*([W] if Wc is None else [W, Wc]), device=self.device)
        return GenoProduct(self.matmul_q(qs[0], None if Wc is None else qs[1], n_slices), e)

    def rmatmul(self, U) -> Tuple[GenoProduct, GenoProduct]:
        """(G^T U, C^T U) for a float matrix [n_ind, k]."""
        (q,), e = geno_quantize(U, device=self.device)
        z, zc = self.rmatmul_q(q)
        return GenoProduct(z, e), GenoProduct(zc, e)

    def stats(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(n, a): per SNP the called individuals and the ALT allele sum over them, exact int64 device tensors [n_snps] (0 for
        a SNP that is not kept): the reverse product of a column of ones."""
        z, zc = self.rmatmul_q(torch.ones((self.n_ind, 1), dtype=torch.int32, device=self.device))
        return zc[:, 0].contiguous(), z[:, 0].contiguous()


def geno_matmul(panel: PackedPanel, W, Wc=None, keep=None) -> GenoProduct:
    """One-shot ``GenoOperator(panel, keep).matmul(W, Wc)``."""
    return GenoOperator(panel, keep).matmul(W, Wc)


def geno_rmatmul(panel: PackedPanel, U, keep=None) -> Tuple[GenoProduct, GenoProduct]:
    """One-shot ``GenoOperator(panel, keep).rmatmul(U)``."""
    return GenoOperator(panel, keep).rmatmul(U)


def geno_planes_host(codes, keep=None) -> Tuple[np.ndarray, np.ndarray]:
    """(g, c) int64 [n_snps, n_ind] from the allele codes [n_snps, n_hap] (1 = ALT, 0 = REF, anything else = missing): the
    dosage of the called genotypes and the called flag; both 0 at a SNP that ``keep`` drops."""
    x = np.asarray(codes)
    if x.ndim != 2 or x.shape[1] % 2 or x.shape[1] == 0:
        raise _lib.LdxError(f"codes [n_snps, n_hap] with an even n_hap needed, got shape {x.shape}")
    h0, h1 = x[:, 0::2], x[:, 1::2]
    called = ((h0 == 0) | (h0 == 1)) & ((h1 == 0) | (h1 == 1))
    k = _keep_mask(keep, x.shape[0])
    if k is not None:
        called = called & k[:, None]
    g = ((h0 == 1).astype(np.int64) + (h1 == 1).astype(np.int64)) * called
    return g, called.astype(np.int64)


def _host_weights(what: str, q, rows: int) -> np.ndarray:
    q = q.cpu().numpy() if isinstance(q, torch.Tensor) else np.asarray(q)
    if q.ndim != 2 or q.shape[0] != rows or q.dtype.kind not in "iu":
        raise _lib.LdxError(f"{what}: integer weights [{rows}, k] needed, got {q.dtype} {q.shape}")
    # 3 x 2^30 per SNP or individual: int64 sums are exact below 2^63 / (3 x 2^30) rows; Python ints beyond
    return q.astype(np.int64) if rows < (1 << 63) // (3 << GENO_SCALE_BITS) else q.astype(object)


def geno_matmul_host(codes, q_w, q_wc=None, keep=None) -> np.ndarray:
    """Host mirror of GenoOperator.matmul_q in numpy integers: [n_ind, k]."""
    g, c = geno_planes_host(codes, keep)
    y = g.T @ _host_weights("geno_matmul_host", q_w, g.shape[0])
    if q_wc is not None:
        y = y + c.T @ _host_weights("geno_matmul_host", q_wc, g.shape[0])
    return y


def geno_rmatmul_host(codes, q_u, keep=None) -> Tuple[np.ndarray, np.ndarray]:
    """Host mirror of GenoOperator.rmatmul_q in numpy integers: (z, zc), [n_snps, k] each."""
    g, c = geno_planes_host(codes, keep)
    u = _host_weights("geno_rmatmul_host", q_u, g.shape[1])
    return g @ u, c @ u


class _GenoEngine:
    """What polygenic_score and sample_pca need of a panel: the two integer products and the torch device of the elementwise
    steps between them.  The device and the host form differ in nothing else, which is what makes them agree bit for bit."""

    device: torch.device
    n_ind: int
    n_snps: int

    def stats(self) -> Tuple[np.ndarray, np.ndarray]:
        z, zc = self.rmatmul_q(torch.ones((self.n_ind, 1), dtype=torch.int32, device=self.device))
        return zc[:, 0].cpu().numpy(), z[:, 0].cpu().numpy()


class _DeviceEngine(_GenoEngine):
    def __init__(self, panel: PackedPanel, keep=None):
        self.op = GenoOperator(panel, keep)
        self.device, self.n_ind, self.n_snps = panel.device, panel.n_ind, panel.n_snps
        self.matmul_q, self.rmatmul_q = self.op.matmul_q, self.op.rmatmul_q

    def called(self) -> np.ndarray:
        return self.op.called_counts().cpu().numpy()


class _HostEngine(_GenoEngine):
    def __init__(self, codes, keep=None):
        self.g, self.c = geno_planes_host(codes, keep)
        self.device, (self.n_snps, self.n_ind) = torch.device("cpu"), self.g.shape

    def matmul_q(self, q_w, q_wc=None):
        y = self.g.T @ _host_weights("matmul_q", q_w, self.n_snps)
        if q_wc is not None:
            y = y + self.c.T @ _host_weights("matmul_q", q_wc, self.n_snps)
        return torch.from_numpy(np.ascontiguousarray(y.astype(np.int64)))

    def rmatmul_q(self, q_u):
        u = _host_weights("rmatmul_q", q_u, self.n_ind)
        return tuple(torch.from_numpy(np.ascontiguousarray((m @ u).astype(np.int64))) for m in (self.g, self.c))

    def called(self) -> np.ndarray:
        return self.c.sum(axis=0)


def _engine(what: str, source, keep) -> _GenoEngine:
    if isinstance(source, PackedPanel):
        require_gpu()
        _even_n_hap(what, source)
        return _DeviceEngine(source, keep)
    return _HostEngine(source, keep)


def _scale_sums(y: np.ndarray, e: np.ndarray) -> np.ndarray:
    """float64(y) 2^(e - 30) on the host: one conversion, one exact scaling."""
    return y.astype(np.float64) * np.ldexp(1.0, (e - GENO_SCALE_BITS).astype(np.int64))[None, :]


def _allele_freq(n: np.ndarray, a: np.ndarray) -> np.ndarray:
    """p = a / (2 n) in fp64 where n > 0, else 0: one division."""
    return np.where(n > 0, a.astype(np.float64) / np.where(n > 0, 2.0 * n.astype(np.float64), 1.0), 0.0)


@dataclass
class Scores:
    """polygenic_score's result: ``sum`` float64 [n_ind, k], the score sums; ``allele_ct`` int64 [n_ind], twice the kept SNPs
    the individual is called at; ``sums`` / ``exps``: the integers behind ``sum`` (sum = sums 2^(exps - 30))."""

    sum: np.ndarray
    allele_ct: np.ndarray
    sums: np.ndarray
    exps: np.ndarray

    @property
    def avg(self) -> np.ndarray:
        """float64 [n_ind, k]: sum / allele_ct (NaN for an individual without a call)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.sum / self.allele_ct[:, None].astype(np.float64)


def _score(eng: _GenoEngine, beta, impute: str, offset=None) -> Scores:
    if impute not in ("mean", "zero"):
        raise _lib.LdxError(f"polygenic_score: impute must be 'mean' or 'zero' (got {impute!r})")

    def weights(x, what):
        x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        x = np.asarray(x, dtype=np.float64)
        x = x[:, None] if x.ndim == 1 else x
        if x.ndim != 2 or x.shape[0] != eng.n_snps:
            raise _lib.LdxError(f"polygenic_score: {what} must have shape [n_snps] or [n_snps, k] (n_snps = {eng.n_snps}), got {x.shape}")
        return x

    b = weights(beta, "beta")
    o = None if offset is None else weights(offset, "offset")
    if o is not None and o.shape != b.shape:
        raise _lib.LdxError(f"polygenic_score: offset {o.shape} beside beta {b.shape}")
    if impute == "zero":   # sum_i c (g b + o)
        qs, e = geno_quantize(*([b] if o is None else [b, o]), device=eng.device)
        y = eng.matmul_q(qs[0], None if o is None else qs[1]).cpu().numpy()
    else:
        n, a = eng.stats()
        tp = 2.0 * _allele_freq(n, a)
        m = tp[:, None] * b
        # sum_i c (g b + o) + (1 - c) (2p b + o)  =  G b - C (2p b) + sum_i (2p b + o), i over the kept SNPs with calls (p = 0 elsewhere)
        qs, e = geno_quantize(*([b, m] if o is None else [b, m, np.where((n > 0)[:, None], o, 0.0)]), device=eng.device)
        const = qs[1].to(torch.int64).sum(dim=0) if o is None else (qs[1].to(torch.int64) + qs[2].to(torch.int64)).sum(dim=0)
        y = (eng.matmul_q(qs[0], -qs[1]) + const[None, :]).cpu().numpy()
    e = e.cpu().numpy()
    return Scores(_scale_sums(y, e), 2 * eng.called().astype(np.int64), y, e)


def polygenic_score(panel: PackedPanel, beta, keep=None, impute: str = "mean", offset=None) -> Scores:
    """Per-SNP weights applied to the individuals of ``panel`` over the SNPs that pass ``keep`` (PLINK's --score sums; this
    project's own definition).  ``beta``: [n_snps] or [n_snps, k], k <= 64.  ``impute="zero"``: sum = G beta, a missing genotype
    adds nothing; ``"mean"``: a missing genotype of a kept SNP with calls counts as 2 p_i, p_i = a_i / (2 n_i) from
    GenoOperator.stats().  ``offset`` (shaped like beta; default none): a constant per SNP that every genotype counted at it adds --
    a weight given for the REF allele is beta = -w, offset = 2 w.  Everything is summed on integers (geno_quantize, the forward
    product on the matrix cores) and scaled once; polygenic_score_host gives the same bits."""
    return _score(_engine("polygenic_score", panel, keep), beta, impute, offset)


def polygenic_score_host(codes, beta, keep=None, impute: str = "mean", offset=None) -> Scores:
    """Host mirror of polygenic_score on the allele codes [n_snps, n_hap]: the same integers from numpy products."""
    return _score(_HostEngine(codes, keep), beta, impute, offset)


@dataclass
class SamplePCA:
    """sample_pca's result: ``eigenvalues`` float64 [n_pcs] (descending) and ``eigenvectors`` float64 [n_ind, n_pcs] of the
    GRM X X^T / M, each vector with its largest-magnitude entry positive; ``n_used`` = M, the SNPs with a finite weight;
    ``loadings`` float64 [n_snps, n_pcs] = X^T u_j / sqrt(M lambda_j), or None; ``two_p`` and ``inv_sd``: 2 p_i and
    1 / sqrt(v_i) per SNP (0 for a SNP outside the M), which ``project`` applies to other individuals."""

    eigenvalues: np.ndarray
    eigenvectors: np.ndarray
    n_used: int
    loadings: Optional[np.ndarray]
    two_p: np.ndarray
    inv_sd: np.ndarray

    def project(self, other, keep=None) -> np.ndarray:
        """float64 [n_other, n_pcs]: the coordinates of the individuals of ``other`` -- a PackedPanel (device product) or allele
        codes [n_snps, n_hap] (host product), over the same SNPs -- on the components, with this result's p and v: one forward
        product of the scaled loadings; a training individual gets back its eigenvector entries up to the method's error."""
        if self.loadings is None:
            raise _lib.LdxError("SamplePCA.project needs the loadings: run sample_pca(..., loadings=True)")
        eng = _engine("SamplePCA.project", other, keep)
        if eng.n_snps != self.loadings.shape[0]:
            raise _lib.LdxError(f"SamplePCA.project: {eng.n_snps} SNPs beside the loadings' {self.loadings.shape[0]}")
        lam = np.where(self.eigenvalues > 0, self.eigenvalues, np.inf)
        w = (self.loadings * self.inv_sd[:, None]) / np.sqrt(self.n_used * lam)[None, :]
        (q_w, q_c), e = geno_quantize(w, -(self.two_p[:, None] * w), device=eng.device)
        return _scale_sums(eng.matmul_q(q_w, q_c).cpu().numpy(), e.cpu().numpy())


def _pca(eng: _GenoEngine, n_pcs: int, oversample: int, n_iter: int, seed: int, loadings: bool) -> SamplePCA:
    n_ind = eng.n_ind
    if not 1 <= n_pcs <= n_ind:
        raise _lib.LdxError(f"sample_pca: n_pcs must lie in 1..n_ind = {n_ind} (got {n_pcs})")
    L = min(n_ind, n_pcs + int(oversample))
    if oversample < 0 or n_iter < 0 or not 1 <= L <= _lib.GENO_MAX_COLS:
        raise _lib.LdxError(f"sample_pca: n_pcs + oversample must lie in 1..{_lib.GENO_MAX_COLS} and n_iter be >= 0")
    # 1. the SNP weights, in numpy fp64
    n, a = eng.stats()
    p = _allele_freq(n, a)
    v = 2.0 * p * (1.0 - p)
    ok = (n > 0) & (v > 0)
    w = np.where(ok, 1.0 / np.where(ok, v, 1.0), 0.0)
    M = int(np.count_nonzero(w > 0))
    if M == 0:
        raise _lib.LdxError("sample_pca: no polymorphic SNP with calls")
    tp = 2.0 * p
    tp_d = torch.from_numpy(tp).to(eng.device)[:, None]
    w_d = torch.from_numpy(w).to(eng.device)[:, None]

    def reverse(Q):   # Zs - tp o Zcs, every operation rounded once
        (q,), e = geno_quantize(Q, device=eng.device)
        Z, Zc = eng.rmatmul_q(q)
        s = _pow2(e - GENO_SCALE_BITS)[None, :]
        Zs, Zcs = Z.to(torch.float64) * s, Zc.to(torch.float64) * s
        return Zs - tp_d * Zcs

    def apply(Q):     # 3. H = K Q
        T = reverse(Q) * w_d
        (q_t, q_c), e2 = geno_quantize(T, -(tp_d * T), device=eng.device)
        Y = eng.matmul_q(q_t, q_c).cpu().numpy()
        return _scale_sums(Y, e2.cpu().numpy()) / M

    # 2. the start
    Q = np.linalg.qr(np.random.default_rng(seed).standard_normal((n_ind, L)))[0]
    for _ in range(n_iter):                                   # 4.
        Q = np.linalg.qr(apply(Q))[0]
    H = apply(Q)                                              # 5.
    QtH = Q.T @ H
    lam, S = np.linalg.eigh((QtH + QtH.T) / 2.0)
    top = np.argsort(-lam, kind="stable")[:n_pcs]
    lam, U = lam[top], Q @ S[:, top]
    big = np.argmax(np.abs(U), axis=0)                        # the first largest-magnitude entry of each vector
    U = U * np.where(U[big, np.arange(U.shape[1])] < 0, -1.0, 1.0)[None, :]
    rsv = np.sqrt(w)
    load = None
    if loadings:                                              # 6.
        D = reverse(U).cpu().numpy()
        load = (D * rsv[:, None]) / np.sqrt(M * np.where(lam > 0, lam, np.inf))[None, :]
    return SamplePCA(lam, U, M, load, tp, rsv)


def sample_pca(panel: PackedPanel, n_pcs: int = 10, keep=None, oversample: int = 10, n_iter: int = 10, seed: int = 0,
               loadings: bool = False) -> SamplePCA:
    """The top ``n_pcs`` principal components of the individuals of ``panel`` by randomised subspace iteration on the GRM
    K = X X^T / M, X_ia = c_ia (g_ia - 2 p_i) / sqrt(2 p_i (1 - p_i)) over the M kept SNPs with calls and 0 < p < 1 (this
    project's own definition; FastPCA's scheme).  K is never formed: one application is a reverse and a forward genotype
    product on the matrix cores, both on integers, with one elementwise fp64 step on the device between them; the
    n_ind x (n_pcs + oversample) algebra (QR, the small eigenproblem) is numpy on the host.  sample_pca_host runs the same
    steps with host products and gives the same bits."""
    return _pca(_engine("sample_pca", panel, keep), int(n_pcs), int(oversample), int(n_iter), seed, loadings)


def sample_pca_host(codes, n_pcs: int = 10, keep=None, oversample: int = 10, n_iter: int = 10, seed: int = 0,
                    loadings: bool = False) -> SamplePCA:
    """Host mirror of sample_pca on the allele codes [n_snps, n_hap]."""
    return _pca(_HostEngine(codes, keep), int(n_pcs), int(oversample), int(n_iter), seed, loadings)


# --------------------------------------------------------------------------- weighted sample products, the GRM
WPROD_SCALE_BITS = _lib.WPROD_SCALE_BITS       # a quantised GRM coefficient is rint(2^28 x 2^-e): |q| <= 2^28


def _wprod_weights(what: str, q, rows: int, dev) -> torch.Tensor:
    """The weights of sample_wprod as the entry takes them: a contiguous int32 [rows, 3] tensor on ``dev`` within -2^28 .. 2^28
    (the C entry's precondition, checked here: on the host for a host array, by one device reduction for a device tensor)."""
    t = q if isinstance(q, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(q))
    if t.dtype != torch.int32 or t.ndim != 2 or tuple(t.shape) != (rows, 3):
        raise _lib.LdxError(f"{what}: int32 weights [{rows}, 3] = (q2, q1, q0) needed; got {t.dtype} {tuple(t.shape)}")
    if rows:
        lo, hi = torch.aminmax(t)
        if int(lo.item()) < -_lib.WPROD_MAX_WEIGHT or int(hi.item()) > _lib.WPROD_MAX_WEIGHT:
            raise _lib.LdxError(f"{what}: the weights must lie in -2^28 .. 2^28")
    return t.to(dev).contiguous()


def sample_wprod(panel: PackedPanel, q, keep=None, out: Optional[torch.Tensor] = None, n_slices: Optional[int] = None,
                 store_snps: int = SAMPLE_STORE_SNPS) -> torch.Tensor:
    """S[a, b] = sum_i (q2_i g_ia g_ib + q1_i (g_ia c_ib + c_ia g_ib) + q0_i c_ia c_ib) between the individuals of ``panel`` over
    the SNPs that pass ``keep``: int64 device tensor [n_ind, n_ind], exact (include/ldx.h, "weighted sample products").  ``q``:
    int32 [n_snps, 3] = (q2, q1, q0) per SNP of the panel, each within -2^28 .. 2^28.  The panel is transposed ``store_snps`` SNPs
    at a time as sample_counts does, and each store multiplied on the int8 matrix cores (ldx_sample_wprod_dev).  ``out``: an
    earlier result of the same individuals to add to (chromosomes, chunks of a fileset).  ``n_slices``: the K slices per tile
    (None: the library's choice).  The result does not depend on the order or the split of the SNPs."""
    require_gpu()
    store_snps, keep_d = _store_args("sample_wprod", panel, keep, store_snps)
    n_ind, n_snps, dev = panel.n_ind, panel.n_snps, panel.device
    w = _wprod_weights("sample_wprod", q, n_snps, dev)
    if out is None:
        S, accumulate = torch.empty((n_ind, n_ind), dtype=torch.int64, device=dev), 0
    else:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or tuple(out.shape) != (n_ind, n_ind) or \
                not out.is_contiguous() or out.device != dev:
            raise _lib.LdxError(f"sample_wprod: out must be a contiguous int64 [{n_ind}, {n_ind}] tensor on {dev}")
        S, accumulate = out, 1
    width = min(store_snps, n_snps)
    store = torch.empty(lib.ldx_sample_planes_bytes(n_ind, width), dtype=torch.uint8, device=dev)
    tables = torch.empty(lib.ldx_sample_tables_bytes(n_ind) // 4, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.ldx_sample_wprod_workspace_bytes(width), dtype=torch.uint8, device=dev)
    for begin in range(0, n_snps, store_snps):
        count = min(store_snps, n_snps - begin)
        _planes_launch(panel, keep_d, begin, count, store, tables)
        check(lib.ldx_sample_wprod_dev(store.data_ptr(), tables.data_ptr(), n_ind, count, w.data_ptr() + 12 * begin, S.data_ptr(),
                                       n_ind, accumulate, int(n_slices or 0), *_ws(ws), _stream_ptr()), "ldx_sample_wprod_dev")
        accumulate = 1
    S._keep = (store, tables, ws, w, keep_d)   # alive until the launches are done
    return S


def sample_wprod_host(codes, q, keep=None) -> np.ndarray:
    """Host mirror of sample_wprod in numpy integers, term by term as the definition reads: int64 [n_ind, n_ind] from the allele
    codes [n_snps, n_hap] (Python integers where 9 x 2^28 x n_snps could pass 2^63)."""
    g, c = geno_planes_host(codes, keep)
    q = q.cpu().numpy() if isinstance(q, torch.Tensor) else np.asarray(q)
    if q.ndim != 2 or q.shape != (g.shape[0], 3) or q.dtype.kind not in "iu":
        raise _lib.LdxError(f"sample_wprod_host: integer weights [{g.shape[0]}, 3] needed, got {q.dtype} {q.shape}")
    kind = np.int64 if g.shape[0] < (1 << 63) // (9 << WPROD_SCALE_BITS) else object
    g, c, q = g.astype(kind), c.astype(kind), q.astype(kind)
    q2, q1, q0 = q[:, 0:1], q[:, 1:2], q[:, 2:3]
    return g.T @ (q2 * g) + g.T @ (q1 * c) + c.T @ (q1 * g) + c.T @ (q0 * c)


def grm_exponent(big: float) -> int:
    """The smallest integer e with big 2^-e <= 1 (geno_quantize's rule); 0 for big = 0."""
    big = float(big)
    if not np.isfinite(big) or big < 0:
        raise _lib.LdxError(f"grm_exponent: a finite non-negative value is needed, got {big}")
    if big == 0.0:
        return 0
    mant, e = math.frexp(big)                   # big = mant 2^e, mant in [0.5, 1)
    return e - 1 if mant == 0.5 else e


def grm_coefficients(snp_counts, keep=None, maf_min: Optional[float] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The unquantised half of grm_weights: (x float64 [n_live, 3] = (w, -2 p w, 4 p^2 w), live bool [n_snps]) from the SNP
    counts {called n, het, hom} of geno_snp_counts, every operation rounded once in the order of include/ldx.h."""
    c = snp_counts.cpu().numpy() if isinstance(snp_counts, torch.Tensor) else np.asarray(snp_counts)
    if c.ndim != 2 or c.shape[1] < 3 or c.dtype.kind not in "iu":
        raise _lib.LdxError(f"grm_weights: integer SNP counts [n_snps, 3 or 4] = (called, het, hom ALT) needed, got {c.dtype} {c.shape}")
    if c.dtype == np.int32:
        c = c.view(np.uint32)                   # geno_snp_counts' words
    c = c.astype(np.int64)
    n, s = c[:, 0], c[:, 1] + 2 * c[:, 2]
    two_n = 2 * n
    live = (s > 0) & (s < two_n)                # hence n > 0
    k = _keep_mask(keep, c.shape[0])
    if k is not None:
        live &= k
    if maf_min is not None:
        maf = np.minimum(s, two_n - s).astype(np.float64) / np.where(two_n > 0, two_n, 1).astype(np.float64)
        live &= maf >= float(maf_min)
    p = s[live].astype(np.float64) / two_n[live].astype(np.float64)
    tp = 2.0 * p
    w = 1.0 / (tp * (1.0 - p))
    return np.stack([w, -(tp * w), ((4.0 * p) * p) * w], axis=1).reshape(-1, 3), live


def grm_weights(snp_counts, keep=None, maf_min: Optional[float] = None, exp: Optional[int] = None) -> Tuple[np.ndarray, int, np.ndarray]:
    """The fixed-point GRM coefficients of every SNP (include/ldx.h, "weighted sample products"): (q int32 [n_snps, 3], e, live
    uint8 [n_snps]).  A SNP is live when it is kept, 0 < s < 2 n (s = het + 2 hom) and its MAF is >= ``maf_min``; its
    coefficients (w, -2 p w, 4 p^2 w), p = s / (2 n), w = 1 / (2 p (1 - p)), are quantised with ONE exponent for all 3 n_live
    values -- e = the smallest integer with max |x| 2^-e <= 1, q = rint(x 2^(28 - e)) -- and the other SNPs get (0, 0, 0).
    ``exp``: quantise with this exponent instead (the one of an earlier chunk or of the whole fileset; it must cover every
    value)."""
    x, live = grm_coefficients(snp_counts, keep, maf_min)
    big = float(np.abs(x).max()) if x.size else 0.0
    e = grm_exponent(big) if exp is None else int(exp)
    if abs(e) > _lib.GRM_MAX_EXP or big > math.ldexp(1.0, e):
        raise _lib.LdxError(f"grm_weights: the exponent {e} does not cover the largest coefficient {big}")
    q = np.zeros((live.size, 3), dtype=np.int32)
    q[live] = np.rint(x * math.ldexp(1.0, WPROD_SCALE_BITS - e)).astype(np.int32)
    return q, e, live.astype(np.uint8)


def grm_cell_host(S, N, exp: int) -> np.ndarray:
    """Host mirror of the GRM cell: float32 ((double)S 2^(exp - 28)) / (double)N, -0.0f where N is 0."""
    S, N = np.asarray(S).astype(np.int64), np.asarray(N).astype(np.int64)
    val = ((S.astype(np.float64) * math.ldexp(1.0, int(exp) - WPROD_SCALE_BITS)) / np.where(N > 0, N, 1).astype(np.float64)).astype(np.float32)
    return np.where(N > 0, val, np.float32(-0.0)).astype(np.float32)


def ld_grm_from_sums(S, N, exp: int, device: Optional[torch.device] = None) -> torch.Tensor:
    """The GRM cells of accumulated integers (ldx_grm_cells_dev): float32 device tensor [n_ind, n_ind] from S (int64) and N
    (uint32 values), device tensors or host arrays, so that S and N can be summed over chromosomes before the division."""
    require_gpu()
    dev = device or (S.device if isinstance(S, torch.Tensor) and S.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    s = (S if isinstance(S, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(S).astype(np.int64)))).to(dev)
    if isinstance(N, torch.Tensor):
        n = (N.view(torch.int32) if N.dtype == torch.uint32 else N).to(dev)
    else:
        nn = np.asarray(N).astype(np.int64)
        if nn.size and (int(nn.min()) < 0 or int(nn.max()) >= (1 << 32)):
            raise _lib.LdxError("ld_grm_from_sums: N must hold uint32 values")
        n = torch.from_numpy(np.ascontiguousarray(nn.astype(np.uint32).view(np.int32))).to(dev)
    if n.dtype == torch.int64:
        n = n.to(torch.int32)                   # the low 32 bits: uint32 values
    if s.dtype != torch.int64 or n.dtype != torch.int32 or s.ndim != 2 or s.shape[0] != s.shape[1] or s.shape != n.shape:
        raise _lib.LdxError(f"ld_grm_from_sums: square int64 S and uint32 N of one shape needed, got {tuple(s.shape)} and {tuple(n.shape)}")
    if abs(int(exp)) > _lib.GRM_MAX_EXP:
        raise _lib.LdxError(f"ld_grm_from_sums: exp {exp} outside -{_lib.GRM_MAX_EXP} .. {_lib.GRM_MAX_EXP}")
    s, n = s.contiguous(), n.contiguous()
    m = int(s.shape[0])
    grm = torch.empty((m, m), dtype=torch.float32, device=dev)
    if m:
        check(lib.ldx_grm_cells_dev(s.data_ptr(), m, n.data_ptr(), m, m, int(exp), grm.data_ptr(), m, _stream_ptr()), "ldx_grm_cells_dev")
    return grm


@dataclass
class GrmResult:
    """The genetic relationship matrix as its integers (include/ldx.h, "weighted sample products"): ``S`` int64 [n_ind, n_ind],
    the weighted sums in units of 2^(exp - 28); ``N`` uint32 [n_ind, n_ind], the live SNPs called in both; ``exp``, the shared
    exponent of the coefficients; ``n_live``, the live SNPs so far.  From ld_grm they are device tensors (``counts`` is the
    SampleCounts behind N), from ld_grm_host numpy arrays."""

    S: object
    N: object
    exp: int
    n_live: int
    counts: Optional[SampleCounts] = None

    @property
    def n_ind(self) -> int:
        return int(self.S.shape[0])

    def grm(self):
        """float32 [n_ind, n_ind]: ((double)S 2^(exp - 28)) / (double)N per cell, -0.0f where N is 0 -- GCTA's default: a missing
        call drops out of the pair."""
        if isinstance(self.S, np.ndarray):
            return grm_cell_host(self.S, self.N, self.exp)
        return ld_grm_from_sums(self.S, self.N, self.exp)


def ld_grm(panel: PackedPanel, keep=None, maf_min: Optional[float] = None, out: Optional[GrmResult] = None,
           exp: Optional[int] = None) -> GrmResult:
    """The genetic relationship matrix of the individuals of ``panel`` (gcta --make-grm, plink2 --make-rel) over the SNPs that
    pass ``keep`` and are live (polymorphic among the called, MAF >= ``maf_min``): the SNP counts (geno_snp_counts) give the
    coefficients on the host (grm_weights), sample_wprod the sums S on the int8 matrix cores and sample_counts over the live SNPs
    the jointly called counts N.  ``out``: an earlier result of the same individuals to add to -- chromosomes or chunks of a
    fileset; its exponent is used, and must cover this panel's coefficients.  ``exp``: the exponent to quantise with (None: this
    panel's own, or ``out``'s)."""
    require_gpu()
    _even_n_hap("ld_grm", panel)
    if out is not None:
        if not isinstance(out, GrmResult) or out.counts is None or out.n_ind != panel.n_ind:
            raise _lib.LdxError(f"ld_grm: out must be an earlier ld_grm result of the same {panel.n_ind} individuals")
        if exp is not None and int(exp) != out.exp:
            raise _lib.LdxError(f"ld_grm: exp {exp} beside out's exponent {out.exp}")
        exp = out.exp
    keep_d = _keep_dev(keep, panel.n_snps, panel.device)
    q, e, live = grm_weights(_snp_counts(panel, keep_d), None, maf_min, exp)
    S = sample_wprod(panel, q, keep=live, out=None if out is None else out.S)
    counts = sample_counts(panel, keep=live, out=None if out is None else out.counts)
    return GrmResult(S, counts.n, e, int(live.sum()) + (0 if out is None else out.n_live), counts)


def ld_grm_host(codes, keep=None, maf_min: Optional[float] = None, exp: Optional[int] = None) -> GrmResult:
    """Host mirror of ld_grm on the allele codes [n_snps, n_hap], all numpy: the same integers, and ``grm()`` the same bits."""
    q, e, live = grm_weights(geno_counts_host(codes, keep), None, maf_min, exp)
    S = sample_wprod_host(codes, q, keep=live)
    N = sample_counts_host(codes, keep=live)[0]
    return GrmResult(S, N, e, int(live.sum()))


def grm_cutoff(grm, cutoff: float) -> Tuple[np.ndarray, np.ndarray]:
    """gcta --grm-cutoff: a maximal set of individuals no two of which have a relationship above ``cutoff`` -- king_cutoff's
    greedy rule on this matrix.  Returns (keep bool [n_ind], removed_because_of int64 [n_ind])."""
    return king_cutoff(grm, cutoff)


# --------------------------------------------------------------------------- linear association scan
GLM_MAX_STEPS = 512                            # passes of the tail's continued fraction before flag 6
GLM_EPS = 2.0 ** -50
GLM_FLAGS = {0: "ok", 1: "no call", 2: "constant genotype", 3: "vif", 4: "constant phenotype", 5: "perfect fit",
             6: "iteration cap"}


@dataclass
class GlmDesign:
    """glm_design's result: ``q`` int32 [N, k] and ``exps`` int64 [k], the quantised U = [Q | Y~] (the first ``n_cov`` columns are
    the orthonormal basis of [1 | X], the other ``n_pheno`` the residual phenotypes); ``yy`` float64 [n_pheno], the residual sums
    of squares from the integers; ``df`` = N - n_cov - 1.  All numpy, on the host."""

    q: np.ndarray
    exps: np.ndarray
    yy: np.ndarray
    n_ind: int
    n_cov: int
    n_pheno: int
    df: int


def _glm_matrix(x, what: str, rows: Optional[int] = None) -> np.ndarray:
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if x.dtype.kind not in "fiub":
        raise _lib.LdxError(f"{what} must be real numbers (got {x.dtype})")
    x = np.asarray(x, dtype=np.float64)
    x = x[:, None] if x.ndim == 1 else x
    if x.ndim != 2 or (rows is not None and x.shape[0] != rows):
        raise _lib.LdxError(f"{what} must have shape [{'N' if rows is None else rows}] or [{'N' if rows is None else rows}, k], "
                            f"got {x.shape}")
    if not np.isfinite(x).all():
        raise _lib.LdxError(f"{what} holds a value that is not finite (take the complete rows first: ld_glm(individuals=))")
    return x


def glm_design(Y, covar=None) -> GlmDesign:
    """The design step of the association scan (include/ldx.h, "association scan"), numpy fp64 on the host: D = [1 | covar],
    thin QR, Y~ = Y - Q (Q^T Y), U = [Q | Y~] quantised as one matrix (geno_quantize), yy from the integers.  ``Y``: [N] or
    [N, p]; ``covar``: [N, c'] without an intercept, or None.  Refused: a rank-deficient D (|R_aa| <= 2^-20 max |R|),
    df = N - n_cov - 1 < 1, a non-finite value, more than 64 columns in U."""
    y = _glm_matrix(Y, "glm_design: Y")
    n, p = y.shape
    if p < 1:
        raise _lib.LdxError("glm_design: Y has no column")
    x = np.empty((n, 0)) if covar is None else _glm_matrix(covar, "glm_design: covar", n)
    D = np.concatenate([np.ones((n, 1)), x], axis=1)
    n_cov = D.shape[1]
    if n_cov + p > _lib.GENO_MAX_COLS:
        raise _lib.LdxError(f"glm_design: {n_cov} covariate columns (with the intercept) and {p} phenotypes are more than "
                            f"{_lib.GENO_MAX_COLS} columns in one sweep; batch the phenotypes")
    df = n - n_cov - 1
    if df < 1:
        raise _lib.LdxError(f"glm_design: {n} individuals leave df = N - {n_cov} - 1 = {df} < 1")
    Q, R = np.linalg.qr(D)
    diag = np.abs(np.diag(R))
    if not np.isfinite(R).all() or (diag <= 2.0 ** -20 * np.abs(R).max()).any():
        raise _lib.LdxError("glm_design: the covariates (with the intercept) are rank-deficient: a column is constant or a "
                            "combination of the others")
    yt = y - Q @ (Q.T @ y)
    # a phenotype in the span of [1 | X] leaves only the rounding of the projection, which the quantiser would blow up to full
    # scale: below 2^-40 of the largest |entry| of the phenotype AS GIVEN (not centred) the residual column is zero (flag 4)
    yt[:, np.abs(yt).max(axis=0) <= 2.0 ** -40 * np.abs(y).max(axis=0)] = 0.0
    (q,), e = geno_quantize(np.concatenate([Q, yt], axis=1))
    q, e = q.numpy(), e.numpy()
    # sum_a q^2 exactly, in two limbs: q^2 <= 2^60, so the sums of its low 30 bits and of the rest both fit an int64 for any N here;
    # joined as Python ints and rounded to fp64 once
    sq = q[:, n_cov:].astype(np.int64) ** 2
    lo, hi = (sq & ((1 << 30) - 1)).sum(axis=0), (sq >> 30).sum(axis=0)
    yy = np.asarray([math.ldexp(float((int(hi[j]) << 30) + int(lo[j])), 2 * (int(e[n_cov + j]) - GENO_SCALE_BITS)) for j in range(p)],
                    dtype=np.float64)
    return GlmDesign(q, e, yy, n, n_cov, p, df)


def _glm_cf(a, b, x):
    """The continued fraction of I_x(a, b) by the modified Lentz method, on arrays: (h, converged) -- glm_linear_kernel's steps."""
    tiny = 1e-300
    fix = lambda v: np.where(np.abs(v) < tiny, tiny, v)  # noqa: E731
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c = np.ones_like(x)
    d = 1.0 / fix(1.0 - qab * x / qap)
    h = d.copy()
    done = np.zeros(x.shape, dtype=bool)
    for m in range(1, GLM_MAX_STEPS + 1):
        m2 = 2.0 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 / fix(1.0 + aa * d)
        c = fix(1.0 + aa / c)
        h1 = h * (d * c)
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 / fix(1.0 + aa * d)
        c = fix(1.0 + aa / c)
        dl = d * c
        h = np.where(done, h, h1 * dl)
        done = done | (np.abs(dl - 1.0) <= GLM_EPS)
        if done.all():
            break
    return h, done


def glm_tail_host(t, df: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(p, neglog10_p, converged) of two-sided Student-t statistics ``t`` (finite or +-inf) with ``df`` degrees of freedom: the
    numpy mirror of the kernel's tail (same branches and steps; numpy's log / exp, so equal within rounding, not bit for bit)."""
    t = np.asarray(t, dtype=np.float64)
    a, b = 0.5 * df, 0.5
    ln_beta = math.lgamma(a) + math.lgamma(0.5) - math.lgamma(a + 0.5)
    p, nlp, ok = np.ones(t.shape), np.zeros(t.shape), np.ones(t.shape, dtype=bool)
    with np.errstate(all="ignore"):
        t2 = t * t
        far = np.isinf(t2)
        p[far], nlp[far] = 0.0, np.inf
        go = (t2 > 0.0) & ~far
        if go.any():
            t2 = t2[go]
            den = df + t2
            x, omx = df / den, t2 / den
            front = a * -np.log1p(t2 / df) + b * np.log(omx) - ln_beta
            direct = x < (a + 1.0) / (a + b + 2.0)
            hd, okd = _glm_cf(a, b, np.where(direct, x, 0.0))
            hc, okc = _glm_cf(b, a, np.where(direct, 0.0, omx))
            lnp_d = front - math.log(a) + np.log(hd)
            comp = np.exp(front - math.log(b)) * hc
            lnp = np.where(direct, lnp_d, np.log1p(-comp))
            p[go] = np.where(direct, np.exp(lnp_d), 1.0 - comp)
            nlp[go] = -lnp / 2.302585092994046
            ok[go] = np.where(direct, okd, okc)
    return p, nlp, ok


def glm_linear_host(z, zc, counts, exps, yy, n_ind: int, n_cov: int, max_vif: float = 50.0):
    """The numpy mirror of ldx_glm_linear_dev: (beta, se, t, p, neglog10_p float64 [n_snps, n_pheno], flags uint8) from the int64
    products ``z``, ``zc`` [n_snps, k], the per-SNP ``counts`` [n_snps, 4], the exponents [k] and ``yy`` [n_pheno].  Every
    operation of beta, se, t and the flags is the kernel's, in its order (the h^2 are summed one after the other, not with
    np.sum): those four agree with the device bit for bit."""
    z, zc = np.asarray(z, dtype=np.int64), np.asarray(zc, dtype=np.int64)
    counts = np.asarray(counts).astype(np.int64)
    e, yy = np.asarray(exps, dtype=np.int64), np.asarray(yy, dtype=np.float64)
    n_snps, k = z.shape
    n_pheno = k - n_cov
    df = int(n_ind) - n_cov - 1
    if not (n_cov >= 1 and n_pheno >= 1 and df >= 1 and max_vif > 1.0 and yy.shape == (n_pheno,) and e.shape == (k,)
            and zc.shape == z.shape and counts.shape == (n_snps, 4)):
        raise _lib.LdxError("glm_linear_host: shapes, df or max_vif outside the rules of ldx_glm_linear_dev")
    scale = np.ldexp(1.0, (e - GENO_SCALE_BITS).astype(np.int64))
    n, het, hom = counts[:, 0], counts[:, 1], counts[:, 2]
    s, e2 = het + 2 * hom, het + 4 * hom
    num = n * e2 - s * s
    flag = np.where(n == 0, 1, np.where(num == 0, 2, 0)).astype(np.uint8)
    with np.errstate(all="ignore"):
        nd = np.where(n > 0, n, 1).astype(np.float64)
        mu = s.astype(np.float64) / nd
        gg = num.astype(np.float64) / nd
        acc = np.zeros(n_snps)
        for a in range(n_cov):
            h = (z[:, a].astype(np.float64) - mu * zc[:, a].astype(np.float64)) * scale[a]
            acc = acc + h * h
        d = gg - acc
        flag[(flag == 0) & (d * float(max_vif) < gg)] = 3
        flags = np.repeat(flag[:, None], n_pheno, axis=1)
        flags[(flags == 0) & (yy == 0.0)[None, :]] = 4
        b = (z[:, n_cov:].astype(np.float64) - mu[:, None] * zc[:, n_cov:].astype(np.float64)) * scale[None, n_cov:]
        beta = b / d[:, None]
        s2 = (yy[None, :] - (b * b) / d[:, None]) / float(df)
        flags[(flags == 0) & (s2 <= 0.0)] = 5
        se = np.sqrt(s2 / d[:, None])
        t = beta / se
        fit = flags == 5
        se[fit], t[fit] = 0.0, np.copysign(np.inf, beta[fit])
        live = flags == 0
        p, nlp = np.zeros(t.shape), np.full(t.shape, np.inf)
        p[live], nlp[live], ok = glm_tail_host(t[live], df)
        capped = np.zeros(t.shape, dtype=bool)
        capped[live] = ~ok
        flags[capped] = 6
    dead = (flags != 0) & (flags != 5)
    for out in (beta, se, t, p, nlp):
        out[dead] = np.nan
    return beta, se, t, p, nlp, flags


def geno_counts_host(codes, keep=None) -> np.ndarray:
    """Host mirror of geno_snp_counts on the allele codes: uint32 [n_snps, 4] = {called, het, hom ALT, 0}."""
    g, c = geno_planes_host(codes, keep)
    return np.stack([c.sum(axis=1), (g == 1).sum(axis=1), (g == 2).sum(axis=1), np.zeros(g.shape[0], dtype=np.int64)],
                    axis=1).astype(np.uint32)


def geno_snp_counts(panel: PackedPanel, keep=None) -> torch.Tensor:
    """int32 device tensor [n_snps, 4] (the words are uint32): per SNP the called, heterozygous and homozygous-ALT individuals
    and a zero, from the panel's planes with the reverse genotype product's own words (ldx_geno_snp_counts_dev); the rows of SNPs
    that ``keep`` drops are 0."""
    require_gpu()
    _even_n_hap("geno_snp_counts", panel)
    return _snp_counts(panel, _keep_dev(keep, panel.n_snps, panel.device))


def _snp_counts(panel: PackedPanel, keep_d: Optional[torch.Tensor]) -> torch.Tensor:
    counts = torch.empty((panel.n_snps, 4), dtype=torch.int32, device=panel.device)
    check(lib.ldx_geno_snp_counts_dev(panel.alt.data_ptr(), panel.ref.data_ptr(), panel.n_snps, panel.n_hap, _ptr(keep_d),
                                      counts.data_ptr(), _stream_ptr()), "ldx_geno_snp_counts_dev")
    return counts


@dataclass
class GlmResult:
    """ld_glm's result.  ``beta``, ``se``, ``t``, ``p``, ``neglog10_p``: float64 tensors [n_snps, n_pheno] and ``flags`` uint8
    (GLM_FLAGS; 0 and 5 are finite results, the others NaN) -- on the panel's device, nothing read back until asked for (host
    tensors from ld_glm_host); ``counts`` [n_snps, 4]: called, het, hom ALT per SNP; ``design``: the integers of the design
    step; ``df`` = N - n_cov - 1."""

    beta: torch.Tensor
    se: torch.Tensor
    t: torch.Tensor
    p: torch.Tensor
    neglog10_p: torch.Tensor
    flags: torch.Tensor
    counts: torch.Tensor
    design: GlmDesign
    df: int

    @property
    def n_obs(self) -> np.ndarray:
        """int64 [n_snps]: the individuals called at each SNP (0 for a SNP that is not kept)."""
        return self.counts[:, 0].cpu().numpy().astype(np.int64) & 0xFFFFFFFF

    @property
    def a1_freq(self) -> np.ndarray:
        """float64 [n_snps]: the frequency of the counted allele among the called, (het + 2 hom) / (2 n); 0 without a call."""
        c = self.counts.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        return _allele_freq(c[:, 0], c[:, 1] + 2 * c[:, 2])


def _glm_missing(what: str, missing) -> None:
    if missing == "pairwise":
        raise _lib.LdxError(f"{what}: missing='pairwise' (PLINK's complete-case fit, a refit of every SNP over its called "
                            "individuals) is not implemented; the scan sets a missing genotype to the SNP's mean (missing=None)")
    if missing is not None:
        raise _lib.LdxError(f"{what}: missing must be None (mean imputation), got {missing!r}")


def _glm_columns(individuals, n_ind: int) -> Optional[np.ndarray]:
    if individuals is None:
        return None
    ii = select_index(individuals, n_ind, "individual").astype(np.int64)
    return np.stack([2 * ii, 2 * ii + 1], axis=1).reshape(-1)


def ld_glm(panel: PackedPanel, Y, covar=None, individuals=None, keep=None, max_vif: float = 50.0,
           missing: Optional[str] = None) -> GlmResult:
    """Linear association scan (include/ldx.h, "association scan"; this project's own definition, what PLINK 2 --glm reports for
    a quantitative trait): per SNP that passes ``keep`` the least-squares fit of every column of ``Y`` [N] / [N, p] on the
    genotype, an intercept and ``covar`` [N, c'].  ``individuals`` (index array or mask over the panel's individuals, any order):
    the N individuals the rows of ``Y`` and ``covar`` belong to, taken with PackedPanel.select; default: all, in the panel's
    order.  A missing genotype counts as the SNP's mean over its called individuals -- PLINK refits over the called, so the two
    differ wherever a call is missing; ``missing="pairwise"`` is refused.  One reverse genotype product of the quantised design
    (glm_design; ldx_geno_rmatmul_dev, the launch of GenoOperator.rmatmul_q), one counts launch, one statistics launch;
    ld_glm_host gives beta, se, t and the flags bit for bit."""
    require_gpu()
    _glm_missing("ld_glm", missing)
    _even_n_hap("ld_glm", panel)
    if not float(max_vif) > 1.0:
        raise _lib.LdxError("ld_glm: max_vif must be > 1")
    cols = _glm_columns(individuals, panel.n_ind)
    if cols is not None:
        panel = panel.select(haplotypes=cols)
    des = glm_design(_glm_matrix(Y, "ld_glm: Y", panel.n_ind), None if covar is None else _glm_matrix(covar, "ld_glm: covar", panel.n_ind))
    keep_d = _keep_dev(keep, panel.n_snps, panel.device)
    dev, k, p = panel.device, des.n_cov + des.n_pheno, des.n_pheno
    # the reverse product alone (GenoOperator.rmatmul_q's launch): the operator would first build the individual-major stores of
    # the forward product, which a scan never reads
    z, zc = _rmatmul_launch(panel, keep_d, _geno_weights("ld_glm", des.q, panel.n_ind, dev))
    counts = _snp_counts(panel, keep_d)
    exps, yy = torch.from_numpy(des.exps).to(dev), torch.from_numpy(des.yy).to(dev)
    outs = [torch.empty((panel.n_snps, p), dtype=torch.float64, device=dev) for _ in range(5)]
    flags = torch.empty((panel.n_snps, p), dtype=torch.uint8, device=dev)
    check(lib.ldx_glm_linear_dev(z.data_ptr(), zc.data_ptr(), k, counts.data_ptr(), panel.n_snps, panel.n_ind, des.n_cov, p,
                                 exps.data_ptr(), yy.data_ptr(), float(max_vif), *(o.data_ptr() for o in outs), flags.data_ptr(), p,
                                 _stream_ptr()), "ldx_glm_linear_dev")
    return GlmResult(*outs, flags, counts, des, des.df)


def ld_glm_host(codes, Y, covar=None, individuals=None, keep=None, max_vif: float = 50.0) -> GlmResult:
    """Host mirror of ld_glm on the allele codes [n_snps, n_hap]: the same design, the integer products of geno_rmatmul_host,
    glm_linear_host.  The tensors of the result are on the host."""
    x = np.asarray(codes)
    if x.ndim != 2 or x.shape[1] % 2 or x.shape[1] == 0:
        raise _lib.LdxError(f"ld_glm_host: codes [n_snps, n_hap] with an even n_hap needed, got shape {x.shape}")
    if not float(max_vif) > 1.0:
        raise _lib.LdxError("ld_glm_host: max_vif must be > 1")
    cols = _glm_columns(individuals, x.shape[1] // 2)
    if cols is not None:
        x = x[:, cols]
    n_ind = x.shape[1] // 2
    des = glm_design(_glm_matrix(Y, "ld_glm_host: Y", n_ind), None if covar is None else _glm_matrix(covar, "ld_glm_host: covar", n_ind))
    z, zc = geno_rmatmul_host(x, des.q, keep)
    counts = geno_counts_host(x, keep)
    outs = glm_linear_host(z, zc, counts, des.exps, des.yy, n_ind, des.n_cov, max_vif)
    return GlmResult(*(torch.from_numpy(np.ascontiguousarray(o)) for o in outs), torch.from_numpy(counts.astype(np.int64)), des, des.df)


# --------------------------------------------------------------------------- logistic association scan
LOGIT_DECREMENT = 2.0 ** -60                   # the Newton decrement at which the step applied is the last
FIRTH_STOP = 2.0 ** -88                        # lambda*^2 of the Firth scoring step at which the step applied is the last
FIRTH_MODES = (None, "fallback", "always")
LOGIT_FLAGS = {0: "ok", 1: "no call", 2: "constant genotype", 3: "vif", 4: "unusable phenotype", 5: "no finite maximiser"}


@dataclass
class LogitDesign:
    """logit_design's result, numpy on the host: ``basis`` float64 [n_cov + 1, N], the rows of B = sqrt(N) Q of D = [1 | covar]
    (column-major B); ``y`` uint8 [n_pheno, N]; ``theta0`` float64 [n_pheno, n_cov + 1], the null fit of each phenotype on B, a
    NaN row for a phenotype without a case, without a control or whose null fit did not converge; ``n_cov`` counts the
    covariates WITHOUT the intercept."""

    basis: np.ndarray
    y: np.ndarray
    theta0: np.ndarray
    n_ind: int
    n_cov: int
    n_pheno: int


def _logit_mu(eta):
    """(mu, 1 - mu, w = mu (1 - mu)) of the linear predictor, from e^-|eta|: no cancellation at either end (the kernel's steps)."""
    e = np.exp(-np.abs(eta))
    den = 1.0 + e
    hi, lo = 1.0 / den, e / den
    pos = eta >= 0.0
    return np.where(pos, hi, lo), np.where(pos, lo, hi), hi * lo


def _logit_evaluation(V, yes, theta, gradient: bool):
    """The evaluation that both iterations below begin with, at ``theta``: (mu, r = y - mu, w, L, grad) with L the Cholesky factor
    of the information (V w) V^T and grad = V r (None without ``gradient``); L is None where a sum is not finite or a pivot is
    not > 0, which ends the fit."""
    with np.errstate(all="ignore"):
        mu, om, w = _logit_mu(theta @ V)
        r = np.where(yes, om, -mu)
        info = (V * w) @ V.T
        grad = V @ r if gradient else None
    if not (np.isfinite(info).all() and (grad is None or np.isfinite(grad).all())):
        return mu, r, w, None, grad
    try:
        return mu, r, w, np.linalg.cholesky(info), grad
    except np.linalg.LinAlgError:
        return mu, r, w, None, grad


def _logit_newton(V, y, theta, last_index: int):
    """Undamped Newton on the rows of ``V`` [m, N] from ``theta`` (include/ldx.h, "logistic association scan", Iteration):
    (theta, se of parameter ``last_index``, evaluations, ok)."""
    yes = y != 0
    done = False
    for it in range(1, _lib.LOGIT_MAX_ITER + 1):
        _mu, _r, _w, L, grad = _logit_evaluation(V, yes, theta, True)
        if L is None:
            return theta, np.nan, it, False
        if done:
            return theta, 1.0 / L[last_index, last_index], it, True
        zf = np.linalg.solve(L, grad)
        theta = theta + np.linalg.solve(L.T, zf)
        dec = float(zf @ zf)
        if not np.isfinite(dec):
            return theta, np.nan, it, False
        done = dec <= LOGIT_DECREMENT
    return theta, np.nan, _lib.LOGIT_MAX_ITER, False


def _firth_scoring(V, y, theta, last_index: int, decs: Optional[list] = None):
    """Fisher scoring on Firth's modified score over the rows of ``V`` [m, N] from ``theta`` (include/ldx.h, "Firth logistic
    association scan", Iteration): (theta, se of parameter ``last_index``, evaluations, ok).  ``decs`` collects lambda*^2 of every
    evaluation that takes a step."""
    yes = y != 0
    done = False
    eye = np.eye(V.shape[0])
    # the safeguard: a point whose lambda*^2 is not below that of the point before is given up for one half as far along the same
    # step, and the step length stays halved for the rest of the fit
    length, before, start, step = 1.0, np.inf, theta, None
    for it in range(1, _lib.FIRTH_MAX_ITER + 1):
        mu, r, w, L, _grad = _logit_evaluation(V, yes, theta, False)
        if L is None:
            return theta, np.nan, it, False
        if done:
            return theta, 1.0 / L[last_index, last_index], it, True
        with np.errstate(all="ignore"):
            T = np.linalg.solve(L, eye) @ V                     # M V, M = L^-1: h_a = w_a |M v_a|^2
            h = w * (T * T).sum(axis=0)
            # summed pairwise, as the device sums per lane and then across the lanes: a running sum over thousands of individuals
            # leaves a rounding error in U* that keeps lambda*^2 above the stop constant
            score = (V * (r + h * (0.5 - mu))).sum(axis=1)
            zf = np.linalg.solve(L, score)
            dec = float(zf @ zf)
        if not np.isfinite(dec):
            return theta, np.nan, it, False
        if decs is not None:
            decs.append(dec)
        if dec >= before:                                       # rejected: back to the point before, half as far along its step
            length *= 0.5
        else:
            with np.errstate(all="ignore"):
                start, step, before = theta, np.linalg.solve(L.T, zf), dec
            done = dec <= FIRTH_STOP
        theta = start + length * step
    return theta, np.nan, _lib.FIRTH_MAX_ITER, False


def logit_design(Y, covar=None) -> LogitDesign:
    """The design step of the logistic scan (include/ldx.h, "logistic association scan"), numpy fp64 on the host: D = [1 | covar],
    thin QR with glm_design's refusals, B = sqrt(N) Q, and per phenotype the null fit on B by Newton from 0.  ``Y``: [N] or [N, p]
    of 0 / 1; ``covar``: [N, c'] without an intercept, c' <= 13, or None."""
    y = _glm_matrix(Y, "logit_design: Y")
    n, p = y.shape
    if p < 1:
        raise _lib.LdxError("logit_design: Y has no column")
    if not np.isin(y, (0.0, 1.0)).all():
        raise _lib.LdxError("logit_design: Y must hold 0 (control) and 1 (case) only")
    x = np.empty((n, 0)) if covar is None else _glm_matrix(covar, "logit_design: covar", n)
    n_cov = x.shape[1]
    if n_cov > _lib.LOGIT_MAX_COV:
        raise _lib.LdxError(f"logit_design: {n_cov} covariates are more than LDX_LOGIT_MAX_COV = {_lib.LOGIT_MAX_COV}")
    if n <= n_cov + 2:
        raise _lib.LdxError(f"logit_design: {n} individuals leave no degree of freedom beside the intercept, {n_cov} covariates "
                            "and the genotype")
    Q, R = np.linalg.qr(np.concatenate([np.ones((n, 1)), x], axis=1))
    diag = np.abs(np.diag(R))
    if not np.isfinite(R).all() or (diag <= 2.0 ** -20 * np.abs(R).max()).any():
        raise _lib.LdxError("logit_design: the covariates (with the intercept) are rank-deficient: a column is constant or a "
                            "combination of the others")
    basis = np.ascontiguousarray((math.sqrt(n) * Q).T)
    y8 = np.ascontiguousarray(y.T.astype(np.uint8))
    theta0 = np.full((p, n_cov + 1), np.nan)
    for j in range(p):
        cases = int(y8[j].sum())
        if cases == 0 or cases == n:
            continue
        th, _se, _it, ok = _logit_newton(basis, y8[j], np.zeros(n_cov + 1), n_cov)
        if ok:
            theta0[j] = th
    return LogitDesign(basis, y8, theta0, n, n_cov, p)


def _erfcx_cf(t):
    """erfcx(t) = e^(t^2) erfc(t) for t >= 5 by its continued fraction, 60 terms from the bottom (past full fp64 there)."""
    f = np.zeros_like(t)
    for k in range(60, 0, -1):
        f = (0.5 * k) / (t + f)
    return 0.5641895835477563 / (t + f)


def logit_tail_host(z) -> Tuple[np.ndarray, np.ndarray]:
    """(p, neglog10_p) of the two-sided normal tail of ``z``: p = erfc(|z| / sqrt 2), ln p in log space from |z| / sqrt 2 = 5 on
    -- the numpy mirror of the kernel's tail (math.erfc, and a continued fraction for erfcx)."""
    z = np.asarray(z, dtype=np.float64)
    t = np.abs(z) * 0.7071067811865476
    p = np.vectorize(math.erfc, otypes=[np.float64])(t)
    with np.errstate(all="ignore"):
        far = t >= 5.0
        lnp = np.where(far, np.log(_erfcx_cf(np.where(far, t, 5.0))) - t * t, np.log(p))
        nlp = np.where(t == 0.0, 0.0, -lnp / 2.302585092994046)
    return p, nlp


@dataclass
class LogitResult:
    """ld_glm_logistic's result.  ``beta`` (log odds ratio per ALT allele), ``se``, ``z``, ``p``, ``neglog10_p``: float64 tensors
    [n_snps, n_pheno]; ``flags`` uint8 (LOGIT_FLAGS; every flag but 0 is NaN in all five) and ``n_iter`` uint8, the information
    evaluations -- on the panel's device, nothing read back until asked for (host tensors from ld_glm_logistic_host); ``counts``
    [n_snps, 4]: called, het, hom ALT per SNP; ``design``: the design step's result; ``firth`` uint8, 1 where the cell holds a
    Firth fit (include/ldx.h, "Firth logistic association scan"), None for a scan without ``firth=``."""

    beta: torch.Tensor
    se: torch.Tensor
    z: torch.Tensor
    p: torch.Tensor
    neglog10_p: torch.Tensor
    flags: torch.Tensor
    n_iter: torch.Tensor
    counts: torch.Tensor
    design: LogitDesign
    firth: Optional[torch.Tensor] = None

    n_obs = GlmResult.n_obs
    a1_freq = GlmResult.a1_freq


def _firth_mode(what: str, firth):
    if firth not in FIRTH_MODES:
        raise _lib.LdxError(f"{what}: firth must be None, 'fallback' or 'always', got {firth!r}")
    return firth


def _logit_y(what: str, Y, n_ind: int) -> np.ndarray:
    y = _glm_matrix(Y, f"{what}: Y", n_ind)
    if not np.isin(y, (0.0, 1.0)).all():
        raise _lib.LdxError(f"{what}: Y must hold 0 (control) and 1 (case) only")
    return y


def ld_glm_logistic(panel: PackedPanel, Y, covar=None, individuals=None, keep=None, max_vif: float = 50.0,
                    missing: Optional[str] = None, firth: Optional[str] = None) -> LogitResult:
    """Logistic association scan (include/ldx.h, "logistic association scan"; this project's own definition, what PLINK 2 --glm
    reports for a case/control trait, without its Firth fallback): per SNP that passes ``keep`` the maximum-likelihood logistic
    fit of every 0/1 column of ``Y`` [N] / [N, p] on the genotype, an intercept and ``covar`` [N, c' <= 13].  ``individuals``,
    ``keep``, ``max_vif`` and the mean imputation of missing genotypes are ld_glm's; ``missing="pairwise"`` is refused.  One counts
    launch and one launch of the scan (ldx_glm_logistic_dev: a wave per cell, Newton from the null fit of logit_design, the
    information matrices on the fp64 matrix cores); ld_glm_logistic_host is the same algorithm in numpy.
    ``firth`` (include/ldx.h, "Firth logistic association scan"): "fallback" refits the cells the scan flags 5 by Firth's
    penalised likelihood, a second launch (ldx_glm_firth_dev, mode 1) in stream order behind the first with nothing read back in
    between; "always" fits every cell that way (mode 0 alone).  The result's ``firth`` marks the penalised cells."""
    require_gpu()
    _firth_mode("ld_glm_logistic", firth)
    _glm_missing("ld_glm_logistic", missing)
    _even_n_hap("ld_glm_logistic", panel)
    if not float(max_vif) > 1.0:
        raise _lib.LdxError("ld_glm_logistic: max_vif must be > 1")
    cols = _glm_columns(individuals, panel.n_ind)
    if cols is not None:
        panel = panel.select(haplotypes=cols)
    des = logit_design(_logit_y("ld_glm_logistic", Y, panel.n_ind),
                       None if covar is None else _glm_matrix(covar, "ld_glm_logistic: covar", panel.n_ind))
    keep_d = _keep_dev(keep, panel.n_snps, panel.device)
    dev, p = panel.device, des.n_pheno
    counts = _snp_counts(panel, keep_d)
    basis, y8, theta0 = (torch.from_numpy(a).to(dev) for a in (des.basis, des.y, des.theta0))
    outs = [torch.empty((panel.n_snps, p), dtype=torch.float64, device=dev) for _ in range(5)]
    flags, n_iter = (torch.empty((panel.n_snps, p), dtype=torch.uint8, device=dev) for _ in range(2))
    args = (panel.alt.data_ptr(), panel.ref.data_ptr(), panel.n_snps, panel.n_hap, _ptr(keep_d), counts.data_ptr(),
            basis.data_ptr(), des.n_ind, des.n_cov, y8.data_ptr(), theta0.data_ptr(), p, float(max_vif),
            *(o.data_ptr() for o in outs), flags.data_ptr(), n_iter.data_ptr(), p)
    if firth != "always":
        check(lib.ldx_glm_logistic_dev(*args, _stream_ptr()), "ldx_glm_logistic_dev")
        if firth is None:
            return LogitResult(*outs, flags, n_iter, counts, des)
    mark = torch.empty((panel.n_snps, p), dtype=torch.uint8, device=dev)
    check(lib.ldx_glm_firth_dev(*args, 1 if firth == "fallback" else 0, mark.data_ptr(), _stream_ptr()), "ldx_glm_firth_dev")
    return LogitResult(*outs, flags, n_iter, counts, des, mark)


def ld_glm_logistic_host(codes, Y, covar=None, individuals=None, keep=None, max_vif: float = 50.0,
                         firth: Optional[str] = None) -> LogitResult:
    """Host mirror of ld_glm_logistic on the allele codes [n_snps, n_hap]: the same design step, flags and Newton iteration in
    numpy fp64 (equal within rounding, not bit for bit: numpy's exp and summation order are its own), and for ``firth`` the same
    Fisher scoring on the modified score.  The tensors of the result are on the host."""
    _firth_mode("ld_glm_logistic_host", firth)
    x = np.asarray(codes)
    if x.ndim != 2 or x.shape[1] % 2 or x.shape[1] == 0:
        raise _lib.LdxError(f"ld_glm_logistic_host: codes [n_snps, n_hap] with an even n_hap needed, got shape {x.shape}")
    if not float(max_vif) > 1.0:
        raise _lib.LdxError("ld_glm_logistic_host: max_vif must be > 1")
    cols = _glm_columns(individuals, x.shape[1] // 2)
    if cols is not None:
        x = x[:, cols]
    n_ind = x.shape[1] // 2
    des = logit_design(_logit_y("ld_glm_logistic_host", Y, n_ind),
                       None if covar is None else _glm_matrix(covar, "ld_glm_logistic_host: covar", n_ind))
    g, called = geno_planes_host(x, keep)
    counts = geno_counts_host(x, keep)
    n_snps, p, P = x.shape[0], des.n_pheno, des.n_cov + 1
    c64 = counts.astype(np.int64)
    n, s, e2 = c64[:, 0], c64[:, 1] + 2 * c64[:, 2], c64[:, 1] + 4 * c64[:, 2]
    num = n * e2 - s * s
    outs = [np.full((n_snps, p), np.nan) for _ in range(5)]
    flags, n_iter, mark = (np.zeros((n_snps, p), dtype=np.uint8) for _ in range(3))
    usable = ~np.isnan(des.theta0).any(axis=1)
    V = np.zeros((P + 1, n_ind))
    V[:P] = des.basis
    for i in range(n_snps):
        if n[i] == 0 or num[i] == 0:
            flags[i] = 1 if n[i] == 0 else 2
            continue
        xi = np.where(called[i] != 0, g[i] - float(s[i]) / float(n[i]), 0.0)
        xx = float(num[i]) / float(n[i])
        h = des.basis @ xi
        d = xx - float(((h * h) / float(n_ind)).sum())
        if d * float(max_vif) < xx:
            flags[i] = 3
            continue
        V[P] = xi
        for j in range(p):
            if not usable[j]:
                flags[i, j] = 4
                continue
            start = np.concatenate([des.theta0[j], [0.0]])
            if firth != "always":
                th, se, it, ok = _logit_newton(V, des.y[j], start, P)
                ok = ok and bool(np.isfinite(th[P]) and np.isfinite(se))
            if firth == "always" or (firth == "fallback" and not ok):
                th, se, it, ok = _firth_scoring(V, des.y[j], start, P)
                mark[i, j] = 1
            n_iter[i, j] = it
            if not ok or not (np.isfinite(th[P]) and np.isfinite(se)):
                flags[i, j] = 5
                continue
            outs[0][i, j], outs[1][i, j], outs[2][i, j] = th[P], se, th[P] / se
    live = flags == 0
    outs[3][live], outs[4][live] = logit_tail_host(outs[2][live])
    return LogitResult(*(torch.from_numpy(o) for o in outs), torch.from_numpy(flags), torch.from_numpy(n_iter),
                       torch.from_numpy(counts.astype(np.int64)), des, None if firth is None else torch.from_numpy(mark))


# --------------------------------------------------------------------------- genotype QC and table tests
QC_FLAGS = {0: "ok", 1: "empty", 2: "degenerate", 3: "not a table"}          # ldx_hwe_exact_dev / ldx_fisher_exact_dev
MODEL_TESTS = ("ALLELIC", "TREND", "GENO", "DOM", "REC")                      # the order of ldx_model_tests_dev
MODEL_FLAGS = {0: "ok", 1: "no case or no control", 2: "zero margin", 3: "small cell", 4: "not a table"}
MODEL_MAX_N = _lib.MAX_HAPS // 2                # cases + controls of a model tuple
TIE_BITS = 30                                   # a term is in the tail iff P(k) / P(obs) <= 1 + 2^-30


def _qc_missing(what: str, missing) -> None:
    if missing is not None:
        raise _lib.LdxError(f"{what}: missing={missing!r} has no meaning here: the counts are over each SNP's own called "
                            "individuals (missing must be None)")


def _groups_member(what: str, groups, n_ind: int) -> Tuple[np.ndarray, np.ndarray, list]:
    """(member uint32 [n_ind], sizes int64 [n_groups], labels) of ``groups``: a bool / 0-1 matrix [n_groups, n_ind] (labels
    0 .. n_groups - 1), or a vector [n_ind] of labels expanded to one group per distinct label in sorted order (a NaN label:
    in no group).  None: one group of everybody."""
    if groups is None:
        return np.ones(n_ind, dtype=np.uint32), np.asarray([n_ind], dtype=np.int64), [0]
    g = groups.cpu().numpy() if isinstance(groups, torch.Tensor) else np.asarray(groups)
    if g.ndim == 1:
        if g.shape != (n_ind,):
            raise _lib.LdxError(f"{what}: a label vector needs one entry per individual ({n_ind}), got {g.shape}")
        live = ~np.isnan(g) if g.dtype.kind == "f" else np.ones(n_ind, dtype=bool)
        labels = sorted(set(g[live].tolist()))
        g = np.stack([live & (g == lab) for lab in labels]) if labels else np.zeros((0, n_ind), dtype=bool)
    else:
        if g.ndim != 2 or g.shape[1] != n_ind or (g.dtype != bool and not np.isin(g, (0, 1)).all()):
            raise _lib.LdxError(f"{what}: groups must be a bool / 0-1 matrix [n_groups, {n_ind}] or a label vector [{n_ind}]")
        labels = list(range(g.shape[0]))
    if not 1 <= g.shape[0] <= _lib.QC_MAX_GROUPS:
        raise _lib.LdxError(f"{what}: 1 to {_lib.QC_MAX_GROUPS} groups per call (got {g.shape[0]})")
    g = g.astype(bool)
    member = np.zeros(n_ind, dtype=np.uint32)
    for k in range(g.shape[0]):
        member |= g[k].astype(np.uint32) << np.uint32(k)
    return member, g.sum(axis=1).astype(np.int64), labels


def _member_matrix(member: np.ndarray, n_groups: int) -> np.ndarray:
    return ((member[None, :] >> np.arange(n_groups, dtype=np.uint32)[:, None]) & 1).astype(bool)


def geno_group_counts_host(codes, groups, keep=None) -> Tuple[np.ndarray, np.ndarray]:
    """Host mirror of geno_group_counts on the allele codes: (uint32 [n_snps, n_groups, 4] = {called, het, hom ALT, 0} over each
    group's individuals, the group sizes int64 [n_groups])."""
    g, c = geno_planes_host(codes, keep)
    member, sizes, _ = _groups_member("geno_group_counts_host", groups, g.shape[1])
    m = _member_matrix(member, sizes.size).astype(np.int64).T            # [n_ind, n_groups]
    out = np.stack([c @ m, (g == 1).astype(np.int64) @ m, (g == 2).astype(np.int64) @ m, np.zeros((g.shape[0], sizes.size), dtype=np.int64)],
                   axis=2)
    return out.astype(np.uint32), sizes


def _group_counts(panel: PackedPanel, keep_d: Optional[torch.Tensor], member: np.ndarray, n_groups: int) -> torch.Tensor:
    mem = torch.from_numpy(member.view(np.int32)).to(panel.device)
    counts = torch.empty((panel.n_snps, n_groups, 4), dtype=torch.int32, device=panel.device)
    check(lib.ldx_geno_group_counts_dev(panel.alt.data_ptr(), panel.ref.data_ptr(), panel.n_snps, panel.n_hap, _ptr(keep_d),
                                        mem.data_ptr(), n_groups, counts.data_ptr(), _stream_ptr()), "ldx_geno_group_counts_dev")
    return counts


def geno_group_counts(panel: PackedPanel, groups, keep=None) -> Tuple[torch.Tensor, np.ndarray]:
    """(int32 device tensor [n_snps, n_groups, 4] (the words are uint32), the group sizes int64 [n_groups]): per SNP and group of
    individuals the called, heterozygous and homozygous-ALT individuals and a zero, in ONE pass over the panel's planes
    (ldx_geno_group_counts_dev).  ``groups``: a bool / 0-1 matrix [n_groups, n_ind] -- the groups may overlap, be empty or hold
    everybody -- or a label vector [n_ind], one group per distinct label in sorted order; at most 32 groups.  The rows of SNPs
    that ``keep`` drops are 0.  A group of everybody reproduces geno_snp_counts bit for bit."""
    require_gpu()
    _even_n_hap("geno_group_counts", panel)
    member, sizes, _ = _groups_member("geno_group_counts", groups, panel.n_ind)
    return _group_counts(panel, _keep_dev(keep, panel.n_snps, panel.device), member, int(sizes.size)), sizes


def _int_cols(what: str, named) -> list:
    """The integer arrays of a from_counts call as flat int64 numpy arrays of one length, uint32 values."""
    cols = []
    for name, v in named:
        v = np.ascontiguousarray(v.cpu().numpy() if hasattr(v, "cpu") else v).reshape(-1)
        if v.dtype.kind not in "iu":
            raise _lib.LdxError(f"{what}: {name} must be an integer array, got {v.dtype}")
        if v.size and (int(v.min()) < 0 or int(v.max()) >= (1 << 32)):
            raise _lib.LdxError(f"{what}: {name} must hold uint32 values")
        cols.append(v.astype(np.int64))
    if any(c.size != cols[0].size for c in cols):
        raise _lib.LdxError(f"{what}: {', '.join(n for n, _ in named)} differ in length")
    if cols[0].size == 0:
        raise _lib.LdxError(f"{what}: no tuple given")
    return cols


def _to_dev_u32(cols, dev) -> list:
    return [torch.from_numpy(c.astype(np.uint32).view(np.int32)).to(dev) for c in cols]


def _hwe_check(what: str, n, het, hom) -> None:
    if (het + hom > n).any():
        raise _lib.LdxError(f"{what}: LDX_E_ARG: het + hom > n in a tuple")
    if (n > _lib.QC_MAX_N).any():
        raise _lib.LdxError(f"{what}: LDX_E_ARG: n > LDX_QC_MAX_N = {_lib.QC_MAX_N} in a tuple")


def _fisher_check(what: str, a, b, c, d) -> None:
    if (a + b + c + d > 2 * _lib.QC_MAX_N).any():
        raise _lib.LdxError(f"{what}: LDX_E_ARG: a table holds more than 2 LDX_QC_MAX_N = {2 * _lib.QC_MAX_N} counts")


def _model_check(what: str, R, r1, r2, S, s1, s2) -> None:
    if (r1 + r2 > R).any() or (s1 + s2 > S).any():
        raise _lib.LdxError(f"{what}: LDX_E_ARG: het + hom > n in a tuple")
    if (R + S > MODEL_MAX_N).any():
        raise _lib.LdxError(f"{what}: LDX_E_ARG: more than {MODEL_MAX_N} cases and controls in a tuple")


def _exact_launch(entry: str, cols: list, midp: bool):
    m = int(cols[0].numel())
    dev = cols[0].device
    p = torch.empty(m, dtype=torch.float64, device=dev)
    nlp = torch.empty(m, dtype=torch.float64, device=dev)
    flags = torch.empty(m, dtype=torch.uint8, device=dev)
    check(getattr(lib, entry)(m, *(c.data_ptr() for c in cols), int(bool(midp)), p.data_ptr(), nlp.data_ptr(), flags.data_ptr(),
                              _stream_ptr()), entry)
    return p, nlp, flags


def ld_hwe_from_counts(n, het, hom, midp: bool = False, device: Optional[torch.device] = None):
    """The exact test of Hardy-Weinberg proportions on integer tuples (n called, het, hom ALT) (ldx_hwe_exact_dev; include/ldx.h,
    "genotype QC and table tests"): (p, neglog10_p float64, flags uint8) device tensors [m].  ``midp``: p - P(obs) / 2.  flags
    (QC_FLAGS): 1 n = 0 (NaN), 2 monomorphic (p = 1).  A tuple with het + hom > n or n > 65536 is refused (LDX_E_ARG)."""
    require_gpu()
    dev = device or torch.device("cuda", torch.cuda.current_device())
    cols = _int_cols("ld_hwe_from_counts", (("n", n), ("het", het), ("hom", hom)))
    _hwe_check("ld_hwe_from_counts", *cols)
    return _exact_launch("ldx_hwe_exact_dev", _to_dev_u32(cols, dev), midp)


def ld_fisher_from_counts(a, b, c, d, midp: bool = False, device: Optional[torch.device] = None):
    """Fisher's exact test on the 2 x 2 tables [[a, b], [c, d]] (ldx_fisher_exact_dev), the two-sided tail rule of the HWE test:
    (p, neglog10_p, flags) device tensors [m].  flags: 1 empty table (NaN), 2 a zero row or column margin (p = 1).  A table of
    more than 131072 counts is refused (LDX_E_ARG)."""
    require_gpu()
    dev = device or torch.device("cuda", torch.cuda.current_device())
    cols = _int_cols("ld_fisher_from_counts", (("a", a), ("b", b), ("c", c), ("d", d)))
    _fisher_check("ld_fisher_from_counts", *cols)
    return _exact_launch("ldx_fisher_exact_dev", _to_dev_u32(cols, dev), midp)


def _model_launch(cols: list, min_cell: int):
    m, dev = int(cols[0].numel()), cols[0].device
    chisq, p, nlp = (torch.empty((m, 5), dtype=torch.float64, device=dev) for _ in range(3))
    odds = torch.empty(m, dtype=torch.float64, device=dev)
    flags = torch.empty((m, 5), dtype=torch.uint8, device=dev)
    check(lib.ldx_model_tests_dev(m, *(c.data_ptr() for c in cols), int(min_cell), chisq.data_ptr(), p.data_ptr(), nlp.data_ptr(),
                                  odds.data_ptr(), flags.data_ptr(), _stream_ptr()), "ldx_model_tests_dev")
    return chisq, p, nlp, odds, flags


def _min_cell(what: str, min_cell) -> int:
    if int(min_cell) != min_cell or not 0 <= int(min_cell) < (1 << 32):
        raise _lib.LdxError(f"{what}: min_cell must be an integer in 0 .. 2^32 - 1")
    return int(min_cell)


def ld_model_from_counts(case_n, case_het, case_hom, ctrl_n, ctrl_het, ctrl_hom, min_cell: int = 5,
                         device: Optional[torch.device] = None):
    """The five chi-square tests of ``plink --model`` on integer tuples (ldx_model_tests_dev), MODEL_TESTS in this order: allelic,
    Cochran-Armitage trend, genotypic (2 df), dominant, recessive -- the last two with respect to ALT, not to the minor allele.
    Returns (chisq, p, neglog10_p float64 [m, 5], odds float64 [m] -- the allelic odds ratio --, flags uint8 [m, 5]:
    MODEL_FLAGS) on the device.  model_tests_host gives chisq, odds and the flags bit for bit."""
    require_gpu()
    dev = device or torch.device("cuda", torch.cuda.current_device())
    cols = _int_cols("ld_model_from_counts", (("case_n", case_n), ("case_het", case_het), ("case_hom", case_hom),
                                              ("ctrl_n", ctrl_n), ("ctrl_het", ctrl_het), ("ctrl_hom", ctrl_hom)))
    _model_check("ld_model_from_counts", *cols)
    return _model_launch(_to_dev_u32(cols, dev), _min_cell("ld_model_from_counts", min_cell))


def _tail_ints(weights: list, io: int, midp: bool) -> Tuple[float, float]:
    """(p, neglog10_p) by the two-sided tail rule from the terms' exact integer weights: term k is in the tail iff
    w_k / w_obs <= 1 + 2^-30.  ln p is the difference of two logarithms of Python integers: no range to leave."""
    wo, one = weights[io], 1 << TIE_BITS
    tail = sum(w for w in weights if w * one <= wo * (one + 1))
    total = sum(weights)
    num, den = (2 * tail - wo, 2 * total) if midp else (tail, total)
    if num == den:
        return 1.0, 0.0
    lnp = math.log(num) - math.log(den)
    try:
        p = num / den                      # int / int: correctly rounded, 0.0 on underflow
    except OverflowError:
        p = math.exp(lnp)
    return p, -lnp / 2.302585092994046


def hwe_exact_host(n, het, hom, midp: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Host mirror of ld_hwe_from_counts in Python integers: P(k) ~ 2^k n! / (hA! k! hB!) is 2^k times a multinomial
    coefficient, an exact integer; the first term from binomials, the others by the term ratio.  (p, neglog10_p float64 [m],
    flags uint8 [m]); within the contract, not bit for bit."""
    n, het, hom = _int_cols("hwe_exact_host", (("n", n), ("het", het), ("hom", hom)))
    _hwe_check("hwe_exact_host", n, het, hom)
    p, nlp, flags = np.full(n.size, np.nan), np.full(n.size, np.nan), np.zeros(n.size, dtype=np.uint8)
    for i, (ni, hi, mi) in enumerate(zip(n.tolist(), het.tolist(), hom.tolist())):
        nA = hi + 2 * mi
        nB = 2 * ni - nA
        if ni == 0:
            flags[i] = 1
        elif nA == 0 or nB == 0:
            flags[i], p[i], nlp[i] = 2, 1.0, 0.0
        else:
            k0 = nA & 1
            w = [(math.comb(ni, k0) * math.comb(ni - k0, (nA - k0) // 2)) << k0]
            for k in range(k0, min(nA, nB), 2):      # w_{k+2} = w_k 4 hA hB / ((k + 2)(k + 1)): the division is exact
                w.append(w[-1] * (4 * ((nA - k) // 2) * ((nB - k) // 2)) // ((k + 2) * (k + 1)))
            p[i], nlp[i] = _tail_ints(w, (hi - k0) // 2, midp)
    return p, nlp, flags


def fisher_exact_host(a, b, c, d, midp: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Host mirror of ld_fisher_from_counts in Python integers: P(x) ~ C(r1, x) C(r2, c1 - x)."""
    a, b, c, d = _int_cols("fisher_exact_host", (("a", a), ("b", b), ("c", c), ("d", d)))
    _fisher_check("fisher_exact_host", a, b, c, d)
    p, nlp, flags = np.full(a.size, np.nan), np.full(a.size, np.nan), np.zeros(a.size, dtype=np.uint8)
    for i, (ai, bi, ci, di) in enumerate(zip(a.tolist(), b.tolist(), c.tolist(), d.tolist())):
        r1, r2, c1, c2 = ai + bi, ci + di, ai + ci, bi + di
        if r1 + r2 == 0:
            flags[i] = 1
        elif 0 in (r1, r2, c1, c2):
            flags[i], p[i], nlp[i] = 2, 1.0, 0.0
        else:
            lo, hi = max(0, c1 - r2), min(r1, c1)
            w = [math.comb(r1, lo) * math.comb(r2, c1 - lo)]
            for x in range(lo, hi):                  # w_{x+1} = w_x (r1 - x)(c1 - x) / ((x + 1)(r2 - c1 + x + 1)), exactly
                w.append(w[-1] * ((r1 - x) * (c1 - x)) // ((x + 1) * (r2 - c1 + x + 1)))
            p[i], nlp[i] = _tail_ints(w, ai - lo, midp)
    return p, nlp, flags


def model_tests_host(case_n, case_het, case_hom, ctrl_n, ctrl_het, ctrl_hom, min_cell: int = 5):
    """The numpy mirror of ldx_model_tests_dev: (chisq, p, neglog10_p float64 [m, 5], odds float64 [m], flags uint8 [m, 5]).
    Every integer is exact in int64 and every fp64 operation is the kernel's, in its order: chisq, odds and the flags agree with
    the device bit for bit; the tails are within the contract (logit_tail_host for 1 df)."""
    R, r1, r2, S, s1, s2 = _int_cols("model_tests_host", (("case_n", case_n), ("case_het", case_het), ("case_hom", case_hom),
                                                          ("ctrl_n", ctrl_n), ("ctrl_het", ctrl_het), ("ctrl_hom", ctrl_hom)))
    _model_check("model_tests_host", R, r1, r2, S, s1, s2)
    min_cell = _min_cell("model_tests_host", min_cell)
    m = R.size
    chisq, flags, odds = np.full((m, 5), np.nan), np.zeros((m, 5), dtype=np.uint8), np.full(m, np.nan)
    flags[(R == 0) | (S == 0)] = 1
    live = flags[:, 0] == 0
    N, r0, s0 = R + S, R - r1 - r2, S - s1 - s2
    n0, n1, n2 = r0 + s0, r1 + s1, r2 + s2
    f64 = lambda x: x.astype(np.float64)  # noqa: E731

    def table(t, T, a, b, c, d):
        den = (a + b) * (c + d) * ((a + c) * (b + d))
        ok = live & (den != 0)
        det = a * d - b * c
        with np.errstate(all="ignore"):
            chisq[ok, t] = ((f64(T) * f64(det * det)) / f64(np.where(den != 0, den, 1)))[ok]
        flags[live & (den == 0), t] = 2
        return ok

    a, c = r1 + 2 * r2, s1 + 2 * s2
    b, d = 2 * R - a, 2 * S - c
    ok = table(0, 2 * N, a, b, c, d)
    with np.errstate(all="ignore"):
        odds[ok] = (f64(a * d) / f64(b * c))[ok]
    U = N * (r1 + 2 * r2) - R * (n1 + 2 * n2)
    den = R * S * (N * (n1 + 4 * n2) - (n1 + 2 * n2) * (n1 + 2 * n2))
    ok = live & (den != 0)
    with np.errstate(all="ignore"):
        chisq[ok, 1] = ((f64(N) * f64(U * U)) / f64(np.where(den != 0, den, 1)))[ok]
    flags[live & (den == 0), 1] = 2
    zero = (n0 == 0) | (n1 == 0) | (n2 == 0)
    small = np.zeros(m, dtype=bool)
    for o in (r0, r1, r2, s0, s1, s2):
        small |= o < min_cell
    flags[live & zero, 2] = 2
    flags[live & ~zero & small, 2] = 3
    ok = live & ~zero & ~small
    total = np.zeros(m)
    with np.errstate(all="ignore"):
        for row, cells in ((R, (r0, r1, r2)), (S, (s0, s1, s2))):
            for col, o in zip((n0, n1, n2), cells):
                rc = row * col
                dev = o * N - rc
                total = total + f64(dev * dev) / f64(np.where(ok, N * rc, 1))
    chisq[ok, 2] = total[ok]
    table(3, N, r1 + r2, r0, s1 + s2, s0)
    table(4, N, r2, r0 + r1, s2, s0 + s1)
    p, nlp = np.full((m, 5), np.nan), np.full((m, 5), np.nan)
    for t in (0, 1, 3, 4):
        ok = flags[:, t] == 0
        with np.errstate(all="ignore"):
            p[ok, t], nlp[ok, t] = logit_tail_host(np.sqrt(chisq[ok, t]))
    ok = flags[:, 2] == 0
    p[ok, 2], nlp[ok, 2] = np.exp(-0.5 * chisq[ok, 2]), (0.5 * chisq[ok, 2]) / 2.302585092994046
    return chisq, p, nlp, odds, flags


def _count_cols(counts: torch.Tensor, g: int) -> list:
    """The contiguous uint32 columns called, het, hom ALT of group g of a counts tensor [n_snps, n_groups, 4]."""
    return [counts[:, g, k].contiguous() for k in range(3)]


@dataclass
class HardyResult:
    """ld_hardy's result, per (SNP, group): ``counts`` int32 [n_snps, n_groups, 4] (called, het, hom ALT, 0), ``o_het`` = het / n
    and ``e_het`` = 2 p q with p = (het + 2 hom) / (2 n) (float64, NaN where n = 0), ``p``, ``neglog10_p`` float64 and ``flags``
    uint8 (QC_FLAGS) [n_snps, n_groups] -- on the panel's device; ``sizes``: the groups' individuals; ``labels``: their labels."""

    counts: torch.Tensor
    sizes: np.ndarray
    labels: list
    o_het: torch.Tensor
    e_het: torch.Tensor
    p: torch.Tensor
    neglog10_p: torch.Tensor
    flags: torch.Tensor


def ld_hardy(panel: PackedPanel, groups=None, midp: bool = False, keep=None, missing: Optional[str] = None) -> HardyResult:
    """Genotype counts and the exact Hardy-Weinberg test of every SNP within each group of individuals (PLINK --hardy; this
    project's own definition: include/ldx.h, "genotype QC and table tests"): one geno_group_counts pass, then ld_hwe_from_counts'
    launch on its n_snps x n_groups tuples.  ``groups``: as geno_group_counts (None: everybody).  A SNP that ``keep`` drops has
    zero counts and flag 1."""
    _qc_missing("ld_hardy", missing)
    require_gpu()
    _even_n_hap("ld_hardy", panel)
    member, sizes, labels = _groups_member("ld_hardy", groups, panel.n_ind)
    G = int(sizes.size)
    counts = _group_counts(panel, _keep_dev(keep, panel.n_snps, panel.device), member, G)
    flat = counts.view(-1, 4)
    p, nlp, flags = _exact_launch("ldx_hwe_exact_dev", [flat[:, k].contiguous() for k in range(3)], midp)
    n, het, hom = (flat[:, k].to(torch.float64) for k in range(3))
    a = het + 2.0 * hom
    shape = (panel.n_snps, G)
    return HardyResult(counts, sizes, labels, (het / n).view(shape), ((a * (2.0 * n - a)) / (2.0 * n * n)).view(shape),
                       p.view(shape), nlp.view(shape), flags.view(shape))


def _case_groups(what: str, case, n_ind: int) -> np.ndarray:
    """bool [2, n_ind]: the cases and the controls of a 0 / 1 / NaN vector (NaN: in neither)."""
    v = case.cpu().numpy() if isinstance(case, torch.Tensor) else np.asarray(case)
    v = v.astype(np.float64)
    if v.shape != (n_ind,) or not np.isin(v[~np.isnan(v)], (0.0, 1.0)).all():
        raise _lib.LdxError(f"{what}: case must be a vector [{n_ind}] of 0 (control), 1 (case) and NaN (left out)")
    return np.stack([v == 1.0, v == 0.0])


@dataclass
class ModelResult:
    """ld_model's result.  ``chisq``, ``p``, ``neglog10_p`` float64 [n_snps, 5] and ``flags`` uint8 [n_snps, 5] (MODEL_TESTS,
    MODEL_FLAGS), ``odds`` float64 [n_snps] (allelic), ``fisher_p`` / ``fisher_neglog10_p`` / ``fisher_flags`` [n_snps]: Fisher's
    exact test on the allele counts (None without ``fisher``), ``case_counts`` / ``ctrl_counts`` int32 [n_snps, 4] -- on the
    panel's device; ``n_case``, ``n_ctrl``: the individuals of the two groups."""

    chisq: torch.Tensor
    p: torch.Tensor
    neglog10_p: torch.Tensor
    odds: torch.Tensor
    flags: torch.Tensor
    fisher_p: Optional[torch.Tensor]
    fisher_neglog10_p: Optional[torch.Tensor]
    fisher_flags: Optional[torch.Tensor]
    case_counts: torch.Tensor
    ctrl_counts: torch.Tensor
    n_case: int
    n_ctrl: int


def allele_table(case_counts: torch.Tensor, ctrl_counts: torch.Tensor) -> list:
    """The allelic 2 x 2 table [[a, b], [c, d]] of two counts tensors [n, 4]: ALT and REF alleles of the cases and of the
    controls, four contiguous int32 tensors (uint32 words)."""
    out = []
    for t in (case_counts, ctrl_counts):
        alt = t[:, 1] + 2 * t[:, 2]
        out += [alt.contiguous(), (2 * t[:, 0] - alt).contiguous()]
    return out


def ld_model(panel: PackedPanel, case, midp: bool = False, min_cell: int = 5, fisher: bool = True, keep=None,
             missing: Optional[str] = None) -> ModelResult:
    """The single-SNP case/control table tests of ``plink --model`` and ``--assoc fisher`` (this project's own definition):
    one geno_group_counts pass over cases and controls, ld_model_from_counts' launch on the counts and, with ``fisher``,
    ld_fisher_from_counts' on the allele counts (``midp`` is its).  ``case``: 0 / 1 / NaN per individual, NaN = left out."""
    _qc_missing("ld_model", missing)
    require_gpu()
    _even_n_hap("ld_model", panel)
    groups = _case_groups("ld_model", case, panel.n_ind)
    min_cell = _min_cell("ld_model", min_cell)
    member, sizes, _ = _groups_member("ld_model", groups, panel.n_ind)
    counts = _group_counts(panel, _keep_dev(keep, panel.n_snps, panel.device), member, 2)
    cc, uc = counts[:, 0].contiguous(), counts[:, 1].contiguous()
    outs = _model_launch(_count_cols(counts, 0) + _count_cols(counts, 1), min_cell)
    fp = _exact_launch("ldx_fisher_exact_dev", allele_table(cc, uc), midp) if fisher else (None, None, None)
    return ModelResult(*outs, *fp, cc, uc, int(sizes[0]), int(sizes[1]))


@dataclass
class MissingResult:
    """ld_test_missing's result: ``f_miss_case`` / ``f_miss_ctrl`` float64 [n_snps], the missing-call rates of the two groups (NaN
    for an empty group), ``p``, ``neglog10_p``, ``flags`` of Fisher's test on [[missing, called] cases, [missing, called]
    controls], ``called`` int32 [n_snps, 2] -- on the panel's device; ``n_case``, ``n_ctrl``."""

    f_miss_case: torch.Tensor
    f_miss_ctrl: torch.Tensor
    p: torch.Tensor
    neglog10_p: torch.Tensor
    flags: torch.Tensor
    called: torch.Tensor
    n_case: int
    n_ctrl: int


def ld_test_missing(panel: PackedPanel, case, midp: bool = False, missing: Optional[str] = None) -> MissingResult:
    """Missingness by case/control status (PLINK --test-missing): per SNP Fisher's exact test on the called and missing
    individuals of the cases and of the controls."""
    _qc_missing("ld_test_missing", missing)
    require_gpu()
    _even_n_hap("ld_test_missing", panel)
    member, sizes, _ = _groups_member("ld_test_missing", _case_groups("ld_test_missing", case, panel.n_ind), panel.n_ind)
    counts = _group_counts(panel, None, member, 2)
    called = counts[:, :, 0].contiguous()
    nc, nu = int(sizes[0]), int(sizes[1])
    cols = [(nc - called[:, 0]).contiguous(), called[:, 0].contiguous(), (nu - called[:, 1]).contiguous(), called[:, 1].contiguous()]
    p, nlp, flags = _exact_launch("ldx_fisher_exact_dev", cols, midp)
    with np.errstate(all="ignore"):
        fc = cols[0].to(torch.float64) / float(nc) if nc else torch.full_like(p, float("nan"))
        fu = cols[2].to(torch.float64) / float(nu) if nu else torch.full_like(p, float("nan"))
    return MissingResult(fc, fu, p, nlp, flags, called, nc, nu)


@dataclass
class SampleQC:
    """sample_qc's result, per individual over the kept SNPs: ``called``, ``het``, ``hom`` int64 [n_ind] (the integers
    ldx_sample_planes_dev leaves in its tables), ``n_kept`` the kept SNPs, ``e_hom`` float64: the expected homozygous calls
    sum_s called_is e_s, and ``f`` = (O_hom - E_hom) / (called - E_hom) with O_hom = called - het, the inbreeding coefficient of
    ``plink --het`` (NaN where called = E_hom)."""

    called: np.ndarray
    het: np.ndarray
    hom: np.ndarray
    n_kept: int
    e_hom: np.ndarray
    f: np.ndarray

    @property
    def f_miss(self) -> np.ndarray:
        """float64 [n_ind]: 1 - called / n_kept (NaN without a kept SNP)."""
        with np.errstate(all="ignore"):
            return 1.0 - self.called.astype(np.float64) / float(self.n_kept) if self.n_kept else np.full(self.called.size, np.nan)


def het_weights(snp_counts) -> Tuple[np.ndarray, np.ndarray]:
    """(q int32 [n_snps, 1], exps int64 [1]): the per-SNP expected homozygosity e_s = 1 - a (2n - a) / (n (2n - 1)), a = het +
    2 hom over the n called (the unbiased estimate of PLINK --het; 0 where n = 0), as quantised weights of the genotype products
    (geno_quantize's rule, on the host)."""
    c = np.asarray(snp_counts).astype(np.int64) & 0xFFFFFFFF
    n, a = c[:, 0], c[:, 1] + 2 * c[:, 2]
    with np.errstate(all="ignore"):
        e = np.where(n > 0, 1.0 - (a * (2 * n - a)).astype(np.float64) / np.where(n > 0, n * (2 * n - 1), 1).astype(np.float64), 0.0)
    (q,), exps = geno_quantize(torch.from_numpy(e[:, None]), device="cpu")
    return q.numpy(), exps.numpy()


def _sample_f(called, het, y, exps) -> Tuple[np.ndarray, np.ndarray]:
    e_hom = _scale_sums(np.asarray(y, dtype=np.int64).reshape(-1, 1), np.asarray(exps))[:, 0]
    with np.errstate(all="ignore"):
        f = ((called - het).astype(np.float64) - e_hom) / (called.astype(np.float64) - e_hom)
    return e_hom, f


def sample_qc(panel: PackedPanel, keep=None, missing: Optional[str] = None) -> SampleQC:
    """Per individual the called, heterozygous and homozygous-ALT calls over the SNPs that pass ``keep`` (PLINK --missing's
    sample file, --het): the tables of the individual-major stores (GenoOperator), not a recount; the expected homozygosity sum
    is one forward product of the operator with het_weights as its ``wc`` column."""
    _qc_missing("sample_qc", missing)
    require_gpu()
    op = GenoOperator(panel, keep)
    n_ind = panel.n_ind
    pad = (lib.ldx_sample_tables_bytes(n_ind) // 4 - 4) // 3    # the tables: [3][pad] counters, then the kept SNPs (16 bytes)
    tot, n_kept = np.zeros((3, n_ind), dtype=np.int64), 0
    for _, _, _, tables in op._stores:
        t = tables.cpu().numpy().view(np.uint32).astype(np.int64)
        tot += t[:3 * pad].reshape(3, pad)[:, :n_ind]
        n_kept += int(t[3 * pad])
    q, exps = het_weights(_snp_counts(panel, op._keep_d).cpu().numpy())
    y = op.matmul_q(torch.zeros_like(torch.from_numpy(q)), torch.from_numpy(q)).cpu().numpy()
    e_hom, f = _sample_f(tot[0], tot[1], y, exps)
    return SampleQC(tot[0], tot[1], tot[2], n_kept, e_hom, f)


def sample_qc_host(codes, keep=None) -> SampleQC:
    """Host mirror of sample_qc on the allele codes: the same weights, the integer product of geno_matmul_host."""
    g, c = geno_planes_host(codes, keep)
    k = _keep_mask(keep, g.shape[0])
    q, exps = het_weights(geno_counts_host(codes, keep))
    y = geno_matmul_host(codes, np.zeros_like(q), q, keep)
    called, het, hom = c.sum(axis=0), (g == 1).sum(axis=0), (g == 2).sum(axis=0)
    e_hom, f = _sample_f(called, het, y, exps)
    return SampleQC(called, het, hom, int(g.shape[0] if k is None else k.sum()), e_hom, f)


def snp_qc_mask(panel: PackedPanel, maf_min: Optional[float] = None, geno_max: Optional[float] = None,
                hwe_min: Optional[float] = None, hwe_group=None, midp: bool = False, missing: Optional[str] = None) -> torch.Tensor:
    """The variant filters of PLINK --maf / --geno / --hwe as a device uint8 mask [n_snps] that every operator's ``keep=`` takes
    as it stands.  Over all individuals: min(a, 2n - a) >= maf_min 2n with n > 0, and 1 - n / n_ind <= geno_max; over
    ``hwe_group`` (a bool mask or index array over the individuals, e.g. the controls; None: all): the exact HWE p (``midp``:
    its mid-p) >= hwe_min, a SNP without a call in the group failing."""
    _qc_missing("snp_qc_mask", missing)
    require_gpu()
    _even_n_hap("snp_qc_mask", panel)
    n_ind = panel.n_ind
    groups = np.ones((2, n_ind), dtype=bool)
    if hwe_group is not None:
        groups[1] = False
        groups[1, select_index(hwe_group, n_ind, "individual").astype(np.int64)] = True
    member, _, _ = _groups_member("snp_qc_mask", groups, n_ind)
    counts = _group_counts(panel, None, member, 2).to(torch.int64)
    n, a = counts[:, 0, 0], counts[:, 0, 1] + 2 * counts[:, 0, 2]
    ok = torch.ones(panel.n_snps, dtype=torch.bool, device=panel.device)
    if maf_min is not None:
        ok &= (n > 0) & (torch.minimum(a, 2 * n - a).to(torch.float64) >= float(maf_min) * (2 * n).to(torch.float64))
    if geno_max is not None:
        ok &= (n_ind - n).to(torch.float64) <= float(geno_max) * float(n_ind)
    if hwe_min is not None:
        p, _, flags = _exact_launch("ldx_hwe_exact_dev", [counts[:, 1, k].to(torch.int32).contiguous() for k in range(3)], midp)
        ok &= (flags != 1) & (p >= float(hwe_min))
    return ok.to(torch.uint8)


def sample_qc_mask(panel: PackedPanel, mind_max: Optional[float] = None, het_sd: Optional[float] = None, keep=None) -> np.ndarray:
    """The individual filters of PLINK --mind and of the usual heterozygosity check as a bool mask [n_ind] for
    PackedPanel.select (through its haplotypes) and the drivers: 1 - called / kept SNPs <= mind_max, and |F - mean F| <= het_sd
    standard deviations of F (mean and sample sd over the individuals with a finite F; one without fails)."""
    qc = sample_qc(panel, keep)
    ok = np.ones(qc.called.size, dtype=bool)
    if mind_max is not None:
        ok &= qc.f_miss <= float(mind_max)
    if het_sd is not None:
        fin = np.isfinite(qc.f)
        mean, sd = (qc.f[fin].mean(), qc.f[fin].std(ddof=1)) if fin.sum() > 1 else (0.0, 0.0)
        with np.errstate(all="ignore"):
            ok &= fin & (np.abs(qc.f - mean) <= float(het_sd) * sd)
    return ok


# --------------------------------------------------------------------------- epistasis scan (include/ldx.h, "epistasis scan")
EPI_TESTS = tuple(_lib.EPI_TESTS)                  # "allelic", "boost"
EPI_DF = {"allelic": 1, "boost": 4}
EPI_FLAGS = {1: "a group has no jointly called individual", 2: "a zero among the eight allele cells (dir is NaN)",
             4: "the cycle cap was reached", 8: "a two-way margin is 0", 16: "a group total above LDX_MAX_HAPS / 2"}
_EPI_TR = np.array([(k // 9) * 9 + (k % 3) * 3 + (k % 9) // 3 for k in range(18)])   # the table with the SNPs swapped


def _epi_test(what: str, test) -> int:
    if test not in _lib.EPI_TESTS:
        raise _lib.LdxError(f"{what}: test must be one of {EPI_TESTS}, got {test!r}")
    return _lib.EPI_TESTS[test]


def _epi_missing(what: str, missing) -> None:
    if missing is not None and not (isinstance(missing, str) and missing == "pairwise"):
        raise _lib.LdxError(f'{what}: the scan is pairwise-complete; missing must be None or "pairwise", got {missing!r}')


def _epi_tuples(what: str, counts) -> np.ndarray:
    """int64 [18, ...] from the counts argument of the epilogue functions."""
    k = counts.cpu().numpy() if hasattr(counts, "cpu") else np.asarray(counts)
    if k.ndim < 1 or k.shape[0] != 18 or k.dtype.kind not in "iu":
        raise _lib.LdxError(f"{what}: counts must be an integer array [18, ...], got {k.dtype} with shape {k.shape}")
    k = k.astype(np.int64)
    if k.size and int(k.min()) < 0:
        raise _lib.LdxError(f"{what}: counts must not be negative")
    return k


def epi_counts_host(codes_i, codes_j, case) -> np.ndarray:
    """Host mirror of ld_epistasis_counts on the allele codes: int64 [18, n_i, n_j], the 3 x 3 genotype table of every pair in the
    cases (planes 0 .. 8, 3 a + b) and in the controls (9 .. 17) over the individuals called at both SNPs (both codes of
    haplotypes 2k and 2k + 1 in {0, 1}).  float64 GEMMs of 0 / 1 matrices: exact."""
    ci, cj = np.asarray(codes_i), np.asarray(codes_j)
    if ci.ndim != 2 or cj.ndim != 2 or ci.shape[1] != cj.shape[1] or ci.shape[1] % 2:
        raise _lib.LdxError(f"epi_counts_host: two code matrices over the same even number of haplotypes needed, got shapes "
                            f"{ci.shape} and {cj.shape}")
    groups = _case_groups("epi_counts_host", case, ci.shape[1] // 2)

    def planes(c, member):
        ok = (c >= 0) & (c <= 1)
        q = ok[:, 0::2] & ok[:, 1::2] & member[None, :]
        g = (c[:, 0::2] == 1).astype(np.int64) + (c[:, 1::2] == 1).astype(np.int64)
        return [((g == a) & q).astype(np.float64) for a in range(3)]

    out = []
    for member in groups:
        pi, pj = planes(ci, member), planes(cj, member)
        out += [pi[a] @ pj[b].T for a in range(3) for b in range(3)]
    return np.stack(out).astype(np.int64)


def _epi_allele(k: np.ndarray):
    """(L, V, ok) of one group's nine planes [9, ...]: the log odds ratio of the 2 x 2 allele table and its variance."""
    w = np.arange(3)
    n = k.reshape(3, 3, *k.shape[1:])
    N = n.sum(axis=(0, 1))
    A = np.tensordot(w, n.sum(axis=1), 1)
    B = np.tensordot(w, n.sum(axis=0), 1)
    S = np.tensordot(np.outer(w, w).reshape(-1), k, 1)
    a, b, c, d = S, 2 * A - S, 2 * B - S, 4 * N - 2 * A - 2 * B + S
    ok = (a != 0) & (b != 0) & (c != 0) & (d != 0)
    fa, fb, fc, fd = (np.where(ok, x, 1).astype(np.float64) for x in (a, b, c, d))
    L = np.log((fa * fd) / (fb * fc))
    V = (1.0 / fa + 1.0 / fd) + (1.0 / fb + 1.0 / fc)
    return L, V, ok


def epi_allelic_host(counts) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Host mirror of the allelic test (include/ldx.h, LDX_EPI_ALLELIC) on counts [18, ...] in numpy fp64, every operation
    rounded once in the kernel's order: (chisq float64, dir float64, flags uint8), NaN in both under flag 2."""
    k = _epi_tuples("epi_allelic_host", counts)
    (L1, V1, ok1), (L0, V0, ok0) = _epi_allele(k[:9]), _epi_allele(k[9:])
    ok = ok1 & ok0
    with np.errstate(all="ignore"):
        d = np.where(ok, L1 - L0, np.nan)
        z = d / np.sqrt(V1 + V0)
    return z * z, d, np.where(ok, 0, 2).astype(np.uint8)


def epi_boost_host(counts, max_cycles: int = _lib.EPI_MAX_CYCLES) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """Host mirror of the BOOST test (include/ldx.h, LDX_EPI_BOOST) on counts [18, ...]: ``(mu float64 [18, ...], cycles int64,
    chisq float64, flags uint8)``.  The iterative proportional fitting uses + x / in the kernel's order on the kernel's
    orientation of the table, so mu and cycles are the device's bit for bit; chisq goes through numpy's log."""
    k = _epi_tuples("epi_boost_host", counts)
    shape = k.shape[1:]
    k = k.reshape(18, -1)
    m = k.shape[1]
    t = k[_EPI_TR]
    differ = t != k
    first = np.argmax(differ, axis=0)
    cols = np.arange(m)
    swap = differ.any(axis=0) & (t[first, cols] < k[first, cols])
    o = np.where(swap[None, :], t, k).astype(np.float64)
    m_ab = o[:9] + o[9:]
    m_ac = np.stack([[(o[9 * g + 3 * x] + o[9 * g + 3 * x + 1]) + o[9 * g + 3 * x + 2] for x in range(3)] for g in range(2)])
    m_bc = np.stack([[(o[9 * g + x] + o[9 * g + 3 + x]) + o[9 * g + 6 + x] for x in range(3)] for g in range(2)])
    n_grp = (m_ac[:, 0] + m_ac[:, 1]) + m_ac[:, 2]
    _, _, flags2 = epi_allelic_host(k)
    flags = flags2.astype(np.uint8)
    empty = (n_grp[0] == 0.0) | (n_grp[1] == 0.0)
    flags = flags | np.where(empty, 1, 0).astype(np.uint8)
    zero = (m_ab == 0.0).any(axis=0) | (m_ac == 0.0).any(axis=(0, 1)) | (m_bc == 0.0).any(axis=(0, 1))
    flags = flags | np.where(zero & ~empty, 8, 0).astype(np.uint8)
    tol = 2.0 ** -40 * (n_grp[0] + n_grp[1])
    mu = np.ones((18, m))
    cycles = np.zeros(m, dtype=np.int64)
    conv = empty.copy()

    def scale(v, rows, margin):
        s = v[rows[0]] + v[rows[1]] if len(rows) == 2 else (v[rows[0]] + v[rows[1]]) + v[rows[2]]
        nz = s != 0.0
        f = np.where(nz, margin / np.where(nz, s, 1.0), 0.0)
        for r in rows:
            v[r] = v[r] * f

    for _ in range(int(max_cycles)):
        act = np.nonzero(~conv)[0]
        if not act.size:
            break
        v = mu[:, act]
        old = v.copy()
        for c in range(9):
            scale(v, (c, 9 + c), m_ab[c, act])
        for g in range(2):
            for x in range(3):
                scale(v, (9 * g + 3 * x, 9 * g + 3 * x + 1, 9 * g + 3 * x + 2), m_ac[g, x, act])
        for g in range(2):
            for x in range(3):
                scale(v, (9 * g + x, 9 * g + 3 + x, 9 * g + 6 + x), m_bc[g, x, act])
        mu[:, act] = v
        cycles[act] += 1
        conv[act] = np.abs(v - old).max(axis=0) <= tol[act]
    flags = flags | np.where(~conv, 4, 0).astype(np.uint8)
    acc = np.zeros(m)
    with np.errstate(all="ignore"):
        for c in range(18):
            pos = o[c] > 0.0
            acc = acc + np.where(pos, o[c] * np.log(np.where(pos, o[c], 1.0) / np.where(pos, mu[c], 1.0)), 0.0)
    g2 = 2.0 * acc
    chisq = np.where(empty, np.nan, np.where(g2 > 0.0, g2, 0.0))
    mu = np.where(swap[None, :], mu[_EPI_TR], mu)
    mu[:, empty] = np.nan
    return mu.reshape(18, *shape), cycles.reshape(shape), chisq.reshape(shape), flags.reshape(shape)


def epi_tail_host(chisq, test: str = "boost") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(ln_p, p, neglog10_p)`` of a chi-square of ``test``: 1 df through logit_tail_host(sqrt chisq), 4 df in the closed form
    ln p = -x + log1p(x), x = chisq / 2 (include/ldx.h, "epistasis scan").  NaN stays NaN."""
    _epi_test("epi_tail_host", test)
    x = np.asarray(chisq, dtype=np.float64)
    with np.errstate(all="ignore"):
        if test == "allelic":
            _, nlp = logit_tail_host(np.sqrt(x))
            ln_p = -(nlp * 2.302585092994046)
        else:
            h = 0.5 * x
            ln_p = -h + np.log1p(h)
        ln_p = np.where(np.isnan(x), np.nan, ln_p)
        return ln_p, np.exp(ln_p), -ln_p / 2.302585092994046


def epi_chisq_bound(p: float, test: str = "boost") -> np.float32:
    """The float32 chi-square bound of a p threshold: the smallest float32 b > 0 with p(b) <= ``p`` under epi_tail_host, found
    once on the host by bisection -- the scan then keeps a cell by ONE float32 compare, chisq >= b."""
    _epi_test("epi_chisq_bound", test)
    if not 0.0 < float(p) < 1.0:
        raise _lib.LdxError(f"epi_chisq_bound: p must lie in (0, 1), got {p!r}")
    target = math.log(float(p))
    lo, hi = 0.0, 1.0
    while float(epi_tail_host(hi, test)[0]) > target:
        lo, hi = hi, 2.0 * hi
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if float(epi_tail_host(mid, test)[0]) > target:
            lo = mid
        else:
            hi = mid
    b = np.float32(hi)
    while float(epi_tail_host(float(b), test)[0]) > target:
        b = np.nextafter(b, np.float32(np.inf))
    return b


def _epi_tail_dev(chisq: torch.Tensor, test: str) -> torch.Tensor:
    """ln p of a float chi-square tensor, float64 on its device (epi_tail_host's formulas)."""
    x = chisq.to(torch.float64)
    if test == "allelic":
        t = torch.sqrt(x) * 0.7071067811865476
        near = torch.log(torch.special.erfc(t))
        far = torch.log(torch.special.erfcx(torch.clamp(t, min=5.0))) - t * t
        return torch.where(t < 5.0, near, far)
    h = 0.5 * x
    return -h + torch.log1p(h)


@dataclass
class EpiResult:
    """ld_epistasis' matrices on the device: ``chisq`` and ``dir`` float32 [n_i, n_j], ``flags`` uint8 [n_i, n_j] (EPI_FLAGS, the
    OR of the bits); ``p`` / ``neglog10_p`` are computed from ``chisq`` when asked for (float64, epi_tail_host's formulas)."""

    chisq: torch.Tensor
    dir: torch.Tensor
    flags: torch.Tensor
    test: str
    n_case: int
    n_ctrl: int

    @property
    def df(self) -> int:
        return EPI_DF[self.test]

    @property
    def ln_p(self) -> torch.Tensor:
        return _epi_tail_dev(self.chisq, self.test)

    @property
    def p(self) -> torch.Tensor:
        return torch.exp(self.ln_p)

    @property
    def neglog10_p(self) -> torch.Tensor:
        return -self.ln_p / 2.302585092994046


@dataclass
class EpiSummary:
    """The per-SNP summary of ld_epistasis_hits over the rows of panel I, on the device: ``n_tot`` the valid tests of the SNP,
    ``n_sig`` those with chisq >= ``bound_sig``, ``best_chisq`` (float32, NaN where n_tot is 0) the largest chi-square and
    ``best_partner`` (int64, -1 where n_tot is 0) its partner, the smallest index on ties."""

    n_sig: torch.Tensor
    n_tot: torch.Tensor
    best_chisq: torch.Tensor
    best_partner: torch.Tensor
    bound_sig: np.float32


@dataclass
class EpiHits:
    """The pairs of an epistasis scan at or above a chi-square bound (ld_epistasis_hits) as ld_rect_hits' CSR over the rows of
    panel I: ``hits`` int32 [m, 4] = i, j, chisq bits, dir bits, sorted by (i, j).  The self scan holds every pair once, i > j."""

    offsets: torch.Tensor
    hits: torch.Tensor
    n_i: int
    n_j: int
    bound: np.float32
    test: str
    self_scan: bool
    summary: EpiSummary

    @property
    def j(self) -> torch.Tensor:
        return self.hits[:, 1]

    @property
    def chisq(self) -> torch.Tensor:
        return self.hits[:, 2].view(torch.float32)

    @property
    def dir(self) -> torch.Tensor:
        return self.hits[:, 3].view(torch.float32)

    def __len__(self) -> int:
        return int(self.hits.shape[0])

    def pairs(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """(i int64, j int64, chisq float32, dir float32) on the host, sorted by (i, j)."""
        h = self.hits.cpu().numpy()
        return (h[:, 0].astype(np.int64), h[:, 1].astype(np.int64), np.ascontiguousarray(h[:, 2]).view(np.float32),
                np.ascontiguousarray(h[:, 3]).view(np.float32))


class _EpiSide:
    """One SNP set as the scan takes it (ldx_epi_side): the cases' and the controls' panels, made once with PackedPanel.select,
    and their per-SNP count tables.  Holds the tensors alive."""

    def __init__(self, what: str, panel: PackedPanel, groups: np.ndarray):
        self.panels, self.counts = [], []
        for member in groups:
            ind = np.nonzero(member)[0].astype(np.int64)
            sub = panel.select(haplotypes=np.stack([2 * ind, 2 * ind + 1], axis=1).reshape(-1))
            self.panels.append(sub)
            self.counts.append(_snp_counts(sub, None))
        (pc, pu), (cc, cu) = self.panels, self.counts
        self.struct = _lib.EpiSide(pc.alt.data_ptr(), pc.ref.data_ptr(), cc.data_ptr(), pu.alt.data_ptr(), pu.ref.data_ptr(),
                                   cu.data_ptr(), panel.n_snps)

    @property
    def ref(self):
        return ctypes.byref(self.struct)


def _epi_sides(what: str, panel: PackedPanel, case, panel_j: Optional[PackedPanel], missing):
    """The scan operators' argument rules, checked before anything touches the device, and the two sides: (side_i, side_j,
    n_hap_case, n_hap_ctrl); side_j is side_i where ``panel_j`` is None."""
    _epi_missing(what, missing)
    pj = _rect_panels(what, panel, panel_j, True)
    groups = _case_groups(what, case, panel.n_ind)
    sizes = groups.sum(axis=1)
    if not sizes.all():
        raise _lib.LdxError(f"{what}: {int(sizes[0])} cases and {int(sizes[1])} controls: both groups must hold an individual")
    require_gpu()
    side_i = _EpiSide(what, panel, groups)
    side_j = side_i if panel_j is None else _EpiSide(what, pj, groups)
    return side_i, side_j, 2 * int(sizes[0]), 2 * int(sizes[1])


def ld_epistasis(panel: PackedPanel, case, panel_j: Optional[PackedPanel] = None, test: str = "boost",
                 missing: Optional[str] = None) -> EpiResult:
    """The SNP x SNP interaction test of every SNP of ``panel`` against every SNP of ``panel_j`` (None: ``panel`` itself, the full
    square) in a case/control sample: ``test`` "allelic" (plink --fast-epistasis, 1 df) or "boost" (--fast-epistasis boost, the
    likelihood-ratio test of BOOST, 4 df) on the pair's 3 x 3 x 2 genotype table over the individuals called at both SNPs
    (include/ldx.h, "epistasis scan"; ldx_epi_rect_dev; this project's own definition).  ``case``: ld_model's argument, 0 / 1 /
    NaN per individual, NaN = left out.  ``missing``: None or "pairwise", the same thing: the scan is always pairwise-complete."""
    code = _epi_test("ld_epistasis", test)
    side_i, side_j, hc, hu = _epi_sides("ld_epistasis", panel, case, panel_j, missing)
    n_i, n_j, dev = side_i.struct.n_snps, side_j.struct.n_snps, panel.device
    chisq = torch.empty((n_i, n_j), dtype=torch.float32, device=dev)
    dirn = torch.empty((n_i, n_j), dtype=torch.float32, device=dev)
    flags = torch.empty((n_i, n_j), dtype=torch.uint8, device=dev)
    check(lib.ldx_epi_rect_dev(side_i.ref, side_j.ref, hc, hu, code, chisq.data_ptr(), dirn.data_ptr(), flags.data_ptr(), n_j,
                               _stream_ptr()), "ldx_epi_rect_dev")
    return EpiResult(chisq, dirn, flags, test, hc // 2, hu // 2)


def ld_epistasis_counts(panel: PackedPanel, case, panel_j: Optional[PackedPanel] = None,
                        missing: Optional[str] = None) -> torch.Tensor:
    """The 18 integers of every pair as the scan's K loops produced them, before any float: int32 [18, n_i, n_j] on the device,
    cases then controls, 3 a + b within a group (ldx_epi_counts_dev; epi_counts_host is the numpy mirror)."""
    side_i, side_j, hc, hu = _epi_sides("ld_epistasis_counts", panel, case, panel_j, missing)
    n_i, n_j = side_i.struct.n_snps, side_j.struct.n_snps
    out = torch.empty((18, n_i, n_j), dtype=torch.int32, device=panel.device)
    check(lib.ldx_epi_counts_dev(side_i.ref, side_j.ref, hc, hu, out.data_ptr(), n_j, _stream_ptr()), "ldx_epi_counts_dev")
    return out


def ld_epistasis_hits(panel: PackedPanel, case, panel_j: Optional[PackedPanel] = None, test: str = "boost",
                      chisq: Optional[float] = None, p: float = 1e-4, p_sig: float = 1e-2, hit_capacity: Optional[int] = None,
                      missing: Optional[str] = None) -> EpiHits:
    """The pairs of ld_epistasis whose cell is at or above a bound, and the per-SNP summary PLINK writes next to them
    (ldx_epi_hits_dev + ldx_area_finish_ex_dev).  ``panel_j`` None is the SELF scan: every pair i > j once, and the summary
    credits both SNPs of a pair.  The bound is ``chisq`` where given, else epi_chisq_bound(p): a float32 made once on the host
    and returned as ``.bound``; a cell is kept by one float32 compare.  ``p_sig`` is the summary's threshold (``n_sig``), turned
    into ``summary.bound_sig`` the same way.  Buffers and retries are ld_rect_hits'."""
    code = _epi_test("ld_epistasis_hits", test)
    bound = np.float32(chisq) if chisq is not None else epi_chisq_bound(p, test)
    bound_sig = epi_chisq_bound(p_sig, test)
    if not bound > 0.0:
        raise _lib.LdxError(f"ld_epistasis_hits: the chi-square bound must be > 0, got {bound!r}")
    side_i, side_j, hc, hu = _epi_sides("ld_epistasis_hits", panel, case, panel_j, missing)
    n_i, n_j, dev = side_i.struct.n_snps, side_j.struct.n_snps, panel.device
    self_scan = panel_j is None
    n_tot = torch.zeros(n_i, dtype=torch.int32, device=dev)
    n_sig = torch.zeros(n_i, dtype=torch.int32, device=dev)
    best = torch.zeros(n_i, dtype=torch.int64, device=dev)

    def launch(raw, cap, n_hits, _counts):
        for t in (n_tot, n_sig, best):   # a retry starts the summary again
            t.zero_()
        check(lib.ldx_epi_hits_dev(side_i.ref, side_j.ref, hc, hu, code, int(self_scan), float(bound), raw.data_ptr(), cap,
                                   n_hits.data_ptr(), float(bound_sig), n_tot.data_ptr(), n_sig.data_ptr(), best.data_ptr(),
                                   _stream_ptr()), "ldx_epi_hits_dev")

    offsets, hits = _rect_hits_run("ld_epistasis_hits", launch, n_i, n_j, dev, hit_capacity)
    none = n_tot == 0
    bits = (best >> 32).to(torch.int32)
    best_chisq = torch.where(none, torch.full_like(bits, 0x7FC00000), bits).view(torch.float32)
    partner = torch.where(none, torch.full_like(best, -1), 0xFFFFFFFF - (best & 0xFFFFFFFF))
    return EpiHits(offsets, hits, n_i, n_j, bound, test, self_scan, EpiSummary(n_sig, n_tot, best_chisq, partner, bound_sig))


@dataclass
class EpiCells:
    """ld_epistasis_from_counts' outputs on the device, shaped as the counts behind their first axis: ``chisq`` float64,
    ``chisq32`` (the scan's cell), ``dir`` and ``ln_p`` float64, ``flags`` uint8, ``cycles`` int32 and ``mu`` float64 [18, ...]
    (the fitted table; NaN unless boost without flag 1)."""

    chisq: torch.Tensor
    chisq32: torch.Tensor
    dir: torch.Tensor
    ln_p: torch.Tensor
    flags: torch.Tensor
    mu: torch.Tensor
    cycles: torch.Tensor


def ld_epistasis_from_counts(counts, test: str = "boost", device: Optional[torch.device] = None) -> EpiCells:
    """The scan's epilogue alone on tables ``counts`` [18, ...] (ld_epistasis_counts' order) -- the device function of the scan's
    kernel (ldx_epi_from_counts_dev).  A table with more than LDX_MAX_HAPS / 2 individuals in a group is refused."""
    code = _epi_test("ld_epistasis_from_counts", test)
    k = _epi_tuples("ld_epistasis_from_counts", counts)
    shape = k.shape[1:]
    k = k.reshape(18, -1)
    if k.size and max(int(k[:9].sum(axis=0).max()), int(k[9:].sum(axis=0).max())) > _lib.MAX_HAPS // 2:
        raise _lib.LdxError(f"ld_epistasis_from_counts: LDX_E_ARG: a group total above LDX_MAX_HAPS / 2 = {_lib.MAX_HAPS // 2}")
    m = k.shape[1]
    if m == 0:
        raise _lib.LdxError("ld_epistasis_from_counts: no table given")
    require_gpu()
    dev = device or (counts.device if isinstance(counts, torch.Tensor) and counts.is_cuda else
                     torch.device("cuda", torch.cuda.current_device()))
    tuples = torch.from_numpy(np.ascontiguousarray(k.T).astype(np.uint32).view(np.int32)).to(dev)
    e = lambda dt, *s: torch.empty((m, *s), dtype=dt, device=dev)  # noqa: E731
    chisq, chisq32, dirn, ln_p = e(torch.float64), e(torch.float32), e(torch.float64), e(torch.float64)
    flags, mu, cycles = e(torch.uint8), e(torch.float64, 18), e(torch.int32)
    check(lib.ldx_epi_from_counts_dev(m, code, tuples.data_ptr(), chisq.data_ptr(), chisq32.data_ptr(), dirn.data_ptr(),
                                      ln_p.data_ptr(), flags.data_ptr(), mu.data_ptr(), cycles.data_ptr(), _stream_ptr()),
          "ldx_epi_from_counts_dev")
    v = lambda t: t.view(shape)  # noqa: E731
    return EpiCells(v(chisq), v(chisq32), v(dirn), v(ln_p), v(flags), mu.T.contiguous().view(18, *shape), v(cycles))


# --------------------------------------------------------------------------- permutation tests (include/ldx.h, "permutation tests")
MPERM_TESTS = tuple(_lib.PERM_TESTS)             # "allelic", "trend"
MPERM_FLAGS = {0: "ok", 1: "no called case or no called control", 2: "den = 0: the statistic is undefined", 3: "dropped by keep",
               4: "no table has these margins"}
MPERM_MAX_N = _lib.MAX_HAPS // 2                 # individuals with a phenotype


def _mperm_test(what: str, test) -> int:
    if test not in _lib.PERM_TESTS:
        raise _lib.LdxError(f"{what}: test must be one of {MPERM_TESTS}, got {test!r}")
    return _lib.PERM_TESTS[test]


def _mperm_shape(what: str, n: int, n_case: int, n_perm: int, first: int = 0) -> None:
    if int(n_perm) < 1 or int(first) < 0:
        raise _lib.LdxError(f"{what}: n_perm must be >= 1 and first >= 0 (got {n_perm}, {first})")
    if not 2 <= int(n) <= MPERM_MAX_N:
        raise _lib.LdxError(f"{what}: {n} individuals with a phenotype, outside 2 .. {MPERM_MAX_N} (LDX_MAX_HAPS / 2)")
    if not 1 <= int(n_case) <= int(n) - 1:
        raise _lib.LdxError(f"{what}: n_case {n_case} outside 1 .. n - 1 = {int(n) - 1}: both groups must hold an individual")


def perm_labels_host(n: int, n_case: int, n_perm: int, seed: int, first: int = 0) -> np.ndarray:
    """The numpy mirror of perm_labels: bool [n_perm, n], row r the cases of permutation first + r -- the n_case individuals that
    come first in the order of (key(p, k), k), key = synth.key64(seed, i = p, h = k): uint64 keys and a stable argsort."""
    from . import synth

    _mperm_shape("perm_labels_host", n, n_case, n_perm, first)
    p = np.arange(first, first + n_perm, dtype=np.uint64)
    keys = synth.key64(int(seed), p[:, None], np.arange(n, dtype=np.uint64)[None, :])
    order = np.argsort(keys, axis=1, kind="stable")
    out = np.zeros((n_perm, n), dtype=bool)
    np.put_along_axis(out, order[:, :n_case], True, axis=1)
    return out


@dataclass
class PermLabels:
    """The label plane of a block of permutations (include/ldx.h, "permutation tests"): ``plane`` uint8 [ldx_plane_bytes(n_perm,
    2 n)] on the device, permutations as rows, the bit of haplotype slot 2k set iff individual k is a case.  ``seed`` is None for
    a caller's own labels (from_array)."""

    plane: torch.Tensor
    n: int
    n_case: int
    n_perm: int
    seed: Optional[int] = None
    first: int = 0

    @staticmethod
    def from_array(labels, device: Optional[torch.device] = None) -> "PermLabels":
        """A caller's own labels, bool / 0-1 [n_perm, n]; every row must hold the same number of cases.  Packed by the panels' own
        code: code 1 on the even haplotype slot of a case, 0 elsewhere, and the alt plane of that."""
        x = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
        if x.ndim != 2 or (x.dtype != bool and not np.isin(x, (0, 1)).all()):
            raise _lib.LdxError(f"PermLabels.from_array: a bool / 0-1 matrix [n_perm, n] needed, got {x.dtype} with shape {x.shape}")
        x = x.astype(bool)
        sizes = x.sum(axis=1)
        if x.shape[0] < 1 or (sizes != sizes[0]).any():
            raise _lib.LdxError("PermLabels.from_array: every permutation must hold the same number of cases")
        _mperm_shape("PermLabels.from_array", x.shape[1], int(sizes[0]), x.shape[0])
        codes = np.zeros((x.shape[0], 2 * x.shape[1]), dtype=np.int8)
        codes[:, 0::2] = x
        return PermLabels(PackedPanel.from_codes(codes, device).alt, x.shape[1], int(sizes[0]), x.shape[0])

    def to_array(self) -> np.ndarray:
        """bool [n_perm, n]: the plane unpacked on the host."""
        nch = lib.ldx_n_chunks(2 * self.n)
        words = self.plane.cpu().numpy().view(np.uint32).reshape(-1, nch, _lib.SLAB_ROWS, 4)
        rows = words.transpose(0, 2, 1, 3).reshape(-1, nch * 4)[: self.n_perm]
        bits = np.unpackbits(np.ascontiguousarray(rows).view(np.uint8), axis=1, bitorder="little")
        if bits[:, 1::2].any() or bits[:, 2 * self.n:].any():
            raise _lib.LdxError("PermLabels.to_array: a bit on an odd haplotype slot or beyond the individuals")
        return bits[:, 0:2 * self.n:2].astype(bool)


def perm_labels(n: int, n_case: int, n_perm: int, seed: int, first: int = 0, device: Optional[torch.device] = None) -> PermLabels:
    """The labels of permutations first .. first + n_perm - 1 of ``n`` individuals, ``n_case`` of them cases, made on the device
    (ldx_perm_labels_dev): a permutation depends on (seed, its index, n, n_case) alone.  perm_labels_host is the numpy mirror."""
    _mperm_shape("perm_labels", n, n_case, n_perm, first)
    dev = device or require_gpu()
    plane = torch.empty(lib.ldx_plane_bytes(int(n_perm), 2 * int(n)), dtype=torch.uint8, device=dev)
    check(lib.ldx_perm_labels_dev(int(seed) & ((1 << 64) - 1), int(first), int(n_perm), 2 * int(n), int(n_case), plane.data_ptr(),
                                  _stream_ptr()), "ldx_perm_labels_dev")
    return PermLabels(plane, int(n), int(n_case), int(n_perm), int(seed), int(first))


def _mperm_tuples(what: str, n, het, hom, r, a) -> list:
    cols = _int_cols(what, (("n", n), ("het", het), ("hom", hom), ("r", r), ("a", a)))
    N, n1, n2, R, A = cols
    G = n1 + 2 * n2
    if ((N > MPERM_MAX_N) | (n1 + n2 > N) | (R > N) | (A > 2 * R) | (A > G) | (G - A > 2 * (N - R))).any():
        raise _lib.LdxError(f"{what}: LDX_E_ARG: a tuple that no genotype table of at most {MPERM_MAX_N} individuals has as its margins")
    return cols


def mperm_stat_host(n, het, hom, r, a, test: str = "allelic") -> Tuple[np.ndarray, np.ndarray]:
    """The numpy mirror of ld_mperm_from_counts: (chisq float64 [m], flags uint8 [m]: 1 r = 0 or r = n, 2 den = 0) of the tuples
    (n called, het, hom ALT; r called cases, a their ALT alleles).  int64 integers and the kernel's fp64 operations in its order:
    bit for bit the device's, and model_tests_host's chisq of tests 0 and 1 on any table with these margins."""
    code = _mperm_test("mperm_stat_host", test)
    N, n1, n2, R, A = _mperm_tuples("mperm_stat_host", n, het, hom, r, a)
    G, Q2, S = n1 + 2 * n2, n1 + 4 * n2, N - R
    if code == 0:
        b, c = 2 * R - A, G - A
        d = 2 * S - c
        det = A * d - b * c
        den = (A + b) * (c + d) * ((A + c) * (b + d))
        num = (2 * N).astype(np.float64) * (det * det).astype(np.float64)
    else:
        U = N * A - R * G
        den = R * S * (N * Q2 - G * G)
        num = N.astype(np.float64) * (U * U).astype(np.float64)
    flags = np.where((R == 0) | (S == 0), 1, np.where(den == 0, 2, 0)).astype(np.uint8)
    chisq = np.full(N.size, np.nan)
    ok = flags == 0
    chisq[ok] = num[ok] / den[ok].astype(np.float64)
    return chisq, flags


def _mperm_launch(code: int, cols: list) -> Tuple[torch.Tensor, torch.Tensor]:
    m, dev = int(cols[0].numel()), cols[0].device
    chisq = torch.empty(m, dtype=torch.float64, device=dev)
    flags = torch.empty(m, dtype=torch.uint8, device=dev)
    check(lib.ldx_perm_from_counts_dev(m, code, *(c.data_ptr() for c in cols), chisq.data_ptr(), flags.data_ptr(), _stream_ptr()),
          "ldx_perm_from_counts_dev")
    return chisq, flags


def ld_mperm_from_counts(n, het, hom, r, a, test: str = "allelic", device: Optional[torch.device] = None):
    """The permutation scan's epilogue alone on integer tuples (ldx_perm_from_counts_dev): (chisq float64 [m], flags uint8 [m]) on
    the device.  A tuple that no genotype table has as its margins is refused (LDX_E_ARG)."""
    code = _mperm_test("ld_mperm_from_counts", test)
    cols = _mperm_tuples("ld_mperm_from_counts", n, het, hom, r, a)
    require_gpu()
    dev = device or torch.device("cuda", torch.cuda.current_device())
    return _mperm_launch(code, _to_dev_u32(cols, dev))


def mperm_emp2(stat: torch.Tensor, maxima: torch.Tensor) -> torch.Tensor:
    """EMP2 = (#{p : maxima[p] >= stat[i]} + 1) / (R + 1) by one sort and one searchsorted; NaN where stat is."""
    srt = torch.sort(maxima.reshape(-1)).values
    below = torch.searchsorted(srt, torch.nan_to_num(stat, nan=0.0).contiguous(), right=False)   # maxima < stat
    num = (srt.numel() - below + 1).to(torch.float64)
    emp = num / torch.full_like(num, float(srt.numel() + 1))   # tensor by tensor: ONE fp64 division on every device
    return torch.where(torch.isnan(stat), torch.full_like(emp, float("nan")), emp)


@dataclass
class MpermResult:
    """ld_mperm's result (tensors on the panel's device; ld_mperm_host: on the CPU).  ``stat`` float64 [n_snps], the observed
    chi-square (NaN where flagged); ``flags`` uint8 [n_snps] (MPERM_FLAGS); ``n_ge`` int32 [n_snps], the permutations whose cell is
    valid and >= stat, over ``n_perm_total`` permutations (this call's ``n_perm`` and those counted into a shared ``n_ge`` before);
    ``maxima`` float64 [n_perm], the largest valid chi-square of each of THIS call's permutations over the unflagged SNPs seen so
    far (+0.0: none).  ``emp1`` = (n_ge + 1) / (n_perm_total + 1), ``emp2`` = mperm_emp2(stat, maxima); NaN where flagged."""

    stat: torch.Tensor
    flags: torch.Tensor
    n_ge: torch.Tensor
    maxima: torch.Tensor
    n_perm: int
    n_case: int
    n_ctrl: int
    test: str = "allelic"
    n_perm_total: int = 0

    @property
    def emp1(self) -> torch.Tensor:
        num = self.n_ge.to(torch.float64) + 1.0
        e = num / torch.full_like(num, float(self.n_perm_total + 1))   # tensor by tensor: ONE fp64 division on every device
        return torch.where(self.flags == 0, e, torch.full_like(e, float("nan")))

    @property
    def emp2(self) -> torch.Tensor:
        return mperm_emp2(self.stat, self.maxima)


class _MpermRun:
    """What the scan operators share: the argument rules, the sub-panel of the individuals with a phenotype (PackedPanel.select,
    as the epistasis scan), its per-SNP table, the labels and the observed tuples.  Holds the tensors alive."""

    def __init__(self, what: str, panel: PackedPanel, case, n_perm, seed, first, labels, keep, missing):
        _qc_missing(what, missing)
        _even_n_hap(what, panel)
        groups = _case_groups(what, case, panel.n_ind)
        sizes = groups.sum(axis=1)
        self.n_case, self.n_ctrl = int(sizes[0]), int(sizes[1])
        self.n = self.n_case + self.n_ctrl
        if labels is not None:
            if not isinstance(labels, PermLabels):
                labels = PermLabels.from_array(labels, panel.device)
            if (labels.n, labels.n_case) != (self.n, self.n_case) or (n_perm is not None and int(n_perm) != labels.n_perm):
                raise _lib.LdxError(f"{what}: labels of {labels.n_perm} permutations of {labels.n} individuals with {labels.n_case} "
                                    f"cases; the call has {self.n} individuals with a phenotype, {self.n_case} cases"
                                    + ("" if n_perm is None else f", n_perm = {n_perm}"))
        elif n_perm is None:
            raise _lib.LdxError(f"{what}: give n_perm (and seed) or labels")
        _mperm_shape(what, self.n, self.n_case, labels.n_perm if labels is not None else n_perm, first)
        require_gpu()
        self.keep = _keep_mask(keep, panel.n_snps)
        keep_d = _keep_dev(keep, panel.n_snps, panel.device)
        ind = np.nonzero(groups[0] | groups[1])[0].astype(np.int64)
        self.sub = panel if self.n == panel.n_ind else panel.select(haplotypes=np.stack([2 * ind, 2 * ind + 1], axis=1).reshape(-1))
        self.cnt = _snp_counts(self.sub, keep_d)
        self.labels = labels if labels is not None else perm_labels(self.n, self.n_case, int(n_perm), seed, first, panel.device)
        member, _, _ = _groups_member(what, groups, panel.n_ind)
        self.groups = _group_counts(panel, keep_d, member, 2)      # the observed labels: [n_snps, 2, 4]

    def observed(self, code: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(stat, flags) of the observed labels through the scan's own epilogue."""
        g = self.groups
        tot = g[:, 0] + g[:, 1]
        cols = [tot[:, 0], tot[:, 1], tot[:, 2], g[:, 0, 0], g[:, 0, 1] + 2 * g[:, 0, 2]]
        stat, flags = _mperm_launch(code, [c.contiguous() for c in cols])
        if self.keep is not None:
            flags[torch.from_numpy(~self.keep).to(flags.device)] = 3
        return stat, flags

    def head(self) -> tuple:
        s = self.sub
        return (s.alt.data_ptr(), s.ref.data_ptr(), self.cnt.data_ptr(), s.n_snps, s.n_hap, self.labels.plane.data_ptr(),
                self.labels.n_perm, self.n_case)


def ld_mperm(panel: PackedPanel, case, test: str = "allelic", n_perm: Optional[int] = None, seed: int = 0, first: int = 0,
             labels=None, keep=None, maxima: Optional[torch.Tensor] = None, n_ge: Optional[torch.Tensor] = None,
             n_perm_before: int = 0, missing: Optional[str] = None) -> MpermResult:
    """The max(T) permutation test of ``plink --assoc mperm`` / ``--model mperm`` for the allelic or the trend test (this project's
    own definition: include/ldx.h, "permutation tests"; ldx_perm_scan_dev).  ``case``: ld_model's argument, 0 / 1 / NaN per
    individual, NaN = left out.  The labels of permutations ``first`` .. ``first + n_perm - 1`` come from ``seed`` (perm_labels),
    or ``labels`` gives them: a PermLabels or a bool matrix [R, individuals with a phenotype], every row with as many cases as
    ``case``.  Of the SNP x permutation rectangle only ``n_ge`` and ``maxima`` leave the chip.
    ``maxima``: an earlier call's, over the SAME permutations and other SNPs (a chromosome at a time): this call raises it, and
    its emp2 is then over all SNPs so far.  ``n_ge``: an earlier call's, over the SAME SNPs and other permutations, of which
    ``n_perm_before`` were counted: this call adds to it.  Both are changed in place.  A SNP that ``keep`` drops has flag 3."""
    what = "ld_mperm"
    code = _mperm_test(what, test)
    run = _MpermRun(what, panel, case, n_perm, seed, first, labels, keep, missing)
    R, n, dev = run.labels.n_perm, panel.n_snps, panel.device
    if maxima is None:
        maxima = torch.zeros(R, dtype=torch.float64, device=dev)
    elif maxima.dtype != torch.float64 or maxima.shape != (R,) or maxima.device != dev or not maxima.is_contiguous():
        raise _lib.LdxError(f"{what}: maxima must be a contiguous float64 tensor [{R}] on {dev}")
    if n_ge is None:
        n_ge = torch.zeros(n, dtype=torch.int32, device=dev)
    elif n_ge.dtype != torch.int32 or n_ge.shape != (n,) or n_ge.device != dev or not n_ge.is_contiguous():
        raise _lib.LdxError(f"{what}: n_ge must be a contiguous int32 tensor [{n}] on {dev}")
    stat, flags = run.observed(code)
    check(lib.ldx_perm_scan_dev(*run.head(), code, stat.data_ptr(), n_ge.data_ptr(), maxima.data_ptr(), _stream_ptr()),
          "ldx_perm_scan_dev")
    return MpermResult(stat, flags, n_ge, maxima, R, run.n_case, run.n_ctrl, test, R + int(n_perm_before))


def ld_mperm_counts(panel: PackedPanel, case, n_perm: Optional[int] = None, seed: int = 0, first: int = 0, labels=None,
                    missing: Optional[str] = None) -> torch.Tensor:
    """The two integers of every (SNP, permutation) cell as the scan's K loops produced them, before any float: int32 [2, n_snps,
    R] on the device, a (ALT alleles among the permutation's cases) then R (its cases called at the SNP) (ldx_perm_counts_dev).
    For tests and small R."""
    run = _MpermRun("ld_mperm_counts", panel, case, n_perm, seed, first, labels, None, missing)
    R = run.labels.n_perm
    out = torch.empty((2, panel.n_snps, R), dtype=torch.int32, device=panel.device)
    check(lib.ldx_perm_counts_dev(*run.head(), out.data_ptr(), R, _stream_ptr()), "ldx_perm_counts_dev")
    return out


def ld_mperm_host(codes, case, test: str = "allelic", n_perm: Optional[int] = None, seed: int = 0, first: int = 0, labels=None,
                  keep=None) -> MpermResult:
    """The numpy mirror of ld_mperm on the allele codes [n_snps, n_hap]: the same MpermResult with CPU tensors, bit for bit --
    exact integer GEMMs for (a, R) of every cell, mperm_stat_host for the statistic."""
    what = "ld_mperm_host"
    _mperm_test(what, test)
    g, c = geno_planes_host(codes, keep)
    groups = _case_groups(what, case, g.shape[1])
    ind = np.nonzero(groups[0] | groups[1])[0]
    n, n_case = int(ind.size), int(groups[0].sum())
    if labels is None:
        if n_perm is None:
            raise _lib.LdxError(f"{what}: give n_perm (and seed) or labels")
        L = perm_labels_host(n, n_case, int(n_perm), seed, first)
    else:
        L = labels.to_array() if isinstance(labels, PermLabels) else np.asarray(labels).astype(bool)
        if L.ndim != 2 or L.shape[1] != n or (L.sum(axis=1) != n_case).any():
            raise _lib.LdxError(f"{what}: labels must be [R, {n}] with {n_case} cases in every row")
    g, c = g[:, ind], c[:, ind]
    obs = groups[0][ind]
    N, n1, n2 = c.sum(axis=1), (g == 1).sum(axis=1), (g == 2).sum(axis=1)
    stat, flags = mperm_stat_host(N, n1, n2, c[:, obs].sum(axis=1), g[:, obs].sum(axis=1), test)
    k = _keep_mask(keep, g.shape[0])
    if k is not None:
        flags[~k] = 3
    Lf = L.astype(np.float64).T                                   # sums <= 10 240: exact
    a, R = (g.astype(np.float64) @ Lf).astype(np.int64), (c.astype(np.float64) @ Lf).astype(np.int64)
    m, P = a.shape
    rep = lambda v: np.repeat(v, P)  # noqa: E731
    x, f = mperm_stat_host(rep(N), rep(n1), rep(n2), R.reshape(-1), a.reshape(-1), test)
    x, valid = x.reshape(m, P), (f.reshape(m, P) == 0) & (flags == 0)[:, None]
    n_ge = (valid & (x >= np.where(flags == 0, stat, np.inf)[:, None])).sum(axis=1).astype(np.int32)
    maxima = np.where(valid, x, 0.0).max(axis=0) if m else np.zeros(P)
    t = torch.from_numpy
    return MpermResult(t(stat), t(flags), t(n_ge), t(np.ascontiguousarray(maxima, dtype=np.float64)), P, n_case, n - n_case, test, P)


# --------------------------------------------------------------------------- instrumentation
def probe_andpop(blocks: int, threads: int, iters: int) -> torch.Tensor:
    sink = torch.empty(blocks * threads, dtype=torch.int32, device=torch.device("cuda", torch.cuda.current_device()))
    check(lib.ldx_probe_andpop_dev(sink.data_ptr(), blocks, threads, iters, _stream_ptr()), "ldx_probe_andpop_dev")
    return sink
