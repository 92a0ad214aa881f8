"""PackedPanel: the 2-bit/allele SNP x haplotype matrix resident in HBM.

Replaces the per-pair genotype list assembly of the reference (ld_triangle.py:160-186,
ld_area.py:182-187,230-235): every SNP is turned into an ALT bit-row and a REF bit-row once,
in the tiled layout described in include/ldx.h, together with its allele counts
(calc_ld.py:37-40) and frequency vectors (calc_ld.py:41-44).

torch is used only as the owner of device memory and of the HIP stream; all arithmetic runs
in libldx.so.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import check, lib


def _stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def require_gpu() -> torch.device:
    if not torch.cuda.is_available():
        raise _lib.LdxError("ld_tools_amd needs a HIP device (MI355X / gfx950); there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def encode_codes(genotypes) -> np.ndarray:
    """Allele codes as int8 with the membership rule of list.count (calc_ld.py:37-40).

    1 (also 1.0, True) -> 1 = ALT; 0 (0.0, False) -> 0 = REF; anything else (None for a missing
    GT, 2 for a second ALT, strings, NaN) -> 2 = in neither count.  Accepts a sequence (one
    variant) or a 2-D array-like (variants x haplotypes); numeric numpy input takes a
    vectorised path, object input is compared element by element.
    """
    if isinstance(genotypes, (list, tuple)):
        # the common case -- a flat list of small non-negative ints (0 / 1, the odd 2) -- goes through bytes(): ten times
        # faster than numpy's element-by-element conversion; None, floats, nested rows or large values raise and take the
        # general path below
        try:
            out = np.frombuffer(bytes(genotypes), dtype=np.uint8).copy()
            out[out > 1] = 2
            return out.view(np.int8)
        except (TypeError, ValueError):
            pass
        try:                                # still numeric (floats, large or negative ints, nested rows): vectorised
            arr = np.asarray(genotypes)
            if arr.dtype.kind not in "biuf":
                raise TypeError
        except (TypeError, ValueError):    # None, strings, mixed or ragged content: compared element by element as objects
            arr = np.empty(len(genotypes), dtype=object)
            arr[:] = list(genotypes)
            if all(isinstance(v, (list, tuple)) for v in genotypes) and len({len(v) for v in genotypes}) == 1 and genotypes:
                arr = np.array([list(v) for v in genotypes], dtype=object)
    else:
        arr = genotypes if isinstance(genotypes, np.ndarray) else np.asarray(genotypes, dtype=None)
    if arr.dtype == object or arr.dtype.kind in "USV":
        flat = arr.ravel()
        out = np.fromiter((1 if v == 1 else (0 if v == 0 else 2) for v in flat), dtype=np.int8,
                          count=flat.size)
        return out.reshape(arr.shape)
    out = np.full(arr.shape, 2, dtype=np.int8)
    out[arr == 1] = 1
    out[arr == 0] = 0
    return out


def select_index(x, size: int, what: str) -> np.ndarray:
    """A SNP or haplotype selection as uint32 source indices: a boolean mask of length ``size`` gives its set positions in
    ascending order, an integer index list (numpy, list or torch) is kept in its order, repeats included.  Raises LdxError
    for a mask of another length, a non-integer dtype, a negative value, a value >= size and an empty selection.  Pure numpy
    (``what`` names the axis in the messages)."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    arr = np.asarray(x)
    if arr.ndim != 1:
        raise _lib.LdxError(f"select: {what} must be one-dimensional, got shape {arr.shape}")
    if arr.dtype == bool:
        if arr.size != size:
            raise _lib.LdxError(f"select: the {what} mask has {arr.size} entries for {size}")
        arr = np.flatnonzero(arr)
    if arr.size == 0:
        raise _lib.LdxError(f"select: no {what} selected")
    if arr.dtype.kind not in "iu":
        raise _lib.LdxError(f"select: {what} must be integer indices or a boolean mask, not {arr.dtype}")
    lo, hi = int(arr.min()), int(arr.max())
    if lo < 0 or hi >= size:
        raise _lib.LdxError(f"select: {what} index {lo if lo < 0 else hi} outside 0..{size - 1}")
    return np.ascontiguousarray(arr, dtype=np.uint32)


@dataclass
class PackedPanel:
    """Device-resident packed genotype panel (one chromosome / one sample selection)."""

    n_snps: int
    n_hap: int
    alt: torch.Tensor          # uint8 [plane_bytes]   tiled ALT plane
    ref: torch.Tensor          # uint8 [plane_bytes]   tiled REF plane
    acnt: torch.Tensor         # int32 [padded_snps]   count of code 1 per SNP (bit pattern of uint32)
    rcnt: torch.Tensor         # int32 [padded_snps]   count of code 0 per SNP
    fa: torch.Tensor           # float64 [padded_snps] a / n
    fr: torch.Tensor           # float64 [padded_snps] r / n
    q: torch.Tensor            # float64 [padded_snps] fa * fr

    # ------------------------------------------------------------------ construction
    @staticmethod
    def empty(n_snps: int, n_hap: int, device: Optional[torch.device] = None) -> "PackedPanel":
        dev = device or require_gpu()
        if not (1 <= n_hap <= _lib.MAX_HAPS):
            raise _lib.LdxError(f"n_hap={n_hap} outside 1..{_lib.MAX_HAPS} (LDX_MAX_HAPS)")
        if n_snps < 1:
            raise _lib.LdxError("a panel needs at least one SNP")
        pb = lib.ldx_plane_bytes(n_snps, n_hap)
        npad = lib.ldx_padded_snps(n_snps)
        z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
        return PackedPanel(n_snps, n_hap, z(pb, torch.uint8), z(pb, torch.uint8), z(npad, torch.int32),
                           z(npad, torch.int32), z(npad, torch.float64), z(npad, torch.float64),
                           z(npad, torch.float64))

    @staticmethod
    def from_codes(codes, device: Optional[torch.device] = None) -> "PackedPanel":
        """Pack an int8 [n_snps][n_hap] code matrix (numpy or torch, host or device)."""
        dev = device or require_gpu()
        if isinstance(codes, np.ndarray):
            codes = torch.from_numpy(np.ascontiguousarray(codes, dtype=np.int8))
        if codes.dtype != torch.int8 or codes.dim() != 2:
            raise _lib.LdxError("codes must be an int8 matrix [n_snps][n_hap]")
        codes = codes.to(dev)
        if codes.stride(1) != 1:
            codes = codes.contiguous()      # a row-strided view (padded leading dimension) is taken as is
        n_snps, n_hap = codes.shape
        p = PackedPanel.empty(n_snps, n_hap, dev)
        p.pack_from(codes)
        return p

    @staticmethod
    def from_genotypes(rows, device: Optional[torch.device] = None) -> "PackedPanel":
        """Pack per-variant genotype sequences as calc_ld receives them (lists of 0/1/None/...)."""
        rows = list(rows)
        width = max(len(r) for r in rows)
        codes = np.full((len(rows), width), 2, dtype=np.int8)
        for k, r in enumerate(rows):
            codes[k, :len(r)] = encode_codes(list(r))
        return PackedPanel.from_codes(codes, device)

    @staticmethod
    def from_bed(source, keep=None, extract=None, alt: str = "a1", chunk_snps: int = 65536,
                 out: Optional["PackedPanel"] = None, device: Optional[torch.device] = None) -> "PackedPanel":
        """The panel of a PLINK SNP-major ``.bed``, unpacked on the device from the file's own bytes (include/ldx.h,
        ldx_bed_unpack_dev): what ``from_codes(plink.bed_codes_host(rows, n_ind, keep, alt))`` gives, byte for byte, without
        the codes.  ``source``: a ``plink.BedFile``, or ``(rows, n_ind)`` with the rows a uint8 [n_snps][>= ceil(n_ind / 4)]
        host array or device tensor (unit stride along a row; any alignment, any row stride).  ``extract``: a SNP index array
        or mask (``select_index`` rules); those rows' bytes are gathered before the unpack.  ``keep``: an individual index
        array (any order, repeats allowed) or mask over the file's individuals, applied inside the kernel -- the file may hold
        far more individuals than a panel can.  ``alt``: which allele is code 1, "a1" (PLINK's and LDSC's counted allele) or
        "a2".  A host source moves in chunks of ``chunk_snps`` rows (rounded down to a multiple of 128) through pinned
        staging and is unpacked chunk by chunk; ``out``: a panel of the result's shape to write into (every byte of it is
        written)."""
        from . import plink

        dev = device or (out.device if out is not None else require_gpu())
        a2 = plink._alt_is_a2(alt)
        if isinstance(source, plink.BedFile):
            rows, n_ind = source.rows, source.n_ind
        else:
            try:
                rows, n_ind = source
                n_ind = int(n_ind)
            except (TypeError, ValueError) as exc:
                raise _lib.LdxError("from_bed: source must be a BedFile or (rows, n_ind)") from exc
        on_dev = isinstance(rows, torch.Tensor) and rows.is_cuda
        if isinstance(rows, torch.Tensor) and not on_dev:
            rows = rows.numpy()
        nb = plink.row_bytes(n_ind)
        if not on_dev:
            rows = rows if isinstance(rows, np.ndarray) else np.asarray(rows)
        is_u8 = rows.dtype == (torch.uint8 if on_dev else np.uint8)
        if n_ind < 1 or rows.ndim != 2 or not is_u8 or rows.shape[1] < nb or rows.shape[0] < 1:
            raise _lib.LdxError(f"from_bed: rows must be a uint8 matrix [n_snps][>= {nb}] for {n_ind} individuals")
        if extract is not None:
            ei = select_index(extract, rows.shape[0], "SNP")
            rows = rows[torch.from_numpy(ei.astype(np.int64)).to(rows.device)] if on_dev else np.asarray(rows)[ei]
        ki = None if keep is None else select_index(keep, n_ind, "individual")
        n_snps, n_dst = int(rows.shape[0]), n_ind if ki is None else int(ki.size)
        if 2 * n_dst > _lib.MAX_HAPS:
            raise _lib.LdxError(f"from_bed: {n_dst} individuals are {2 * n_dst} haplotypes, more than {_lib.MAX_HAPS} "
                                "(LDX_MAX_HAPS); pass keep= to take a subset")
        if out is None:
            pb, npad = lib.ldx_plane_bytes(n_snps, 2 * n_dst), lib.ldx_padded_snps(n_snps)
            e = lambda n, dt: torch.empty(n, dtype=dt, device=dev)  # noqa: E731  (the calls write every byte)
            out = PackedPanel(n_snps, 2 * n_dst, e(pb, torch.uint8), e(pb, torch.uint8), e(npad, torch.int32),
                              e(npad, torch.int32), e(npad, torch.float64), e(npad, torch.float64), e(npad, torch.float64))
        elif (out.n_snps, out.n_hap) != (n_snps, 2 * n_dst) or out.device != dev:
            raise _lib.LdxError(f"from_bed: out is a {out.n_snps} x {out.n_hap} panel on {out.device}, the file gives "
                                f"{n_snps} x {2 * n_dst} on {dev}")
        kd = None if ki is None else torch.from_numpy(ki.view(np.int32)).to(dev)
        chunk = max(_lib.SLAB_ROWS, int(chunk_snps) // _lib.SLAB_ROWS * _lib.SLAB_ROWS)

        def unpack(block: torch.Tensor, row0: int) -> None:
            ld = block.stride(0) if block.shape[0] > 1 else max(block.stride(0), nb)
            check(lib.ldx_bed_unpack_dev(block.data_ptr(), ld, n_ind, block.shape[0], _ptr(kd), n_dst, int(a2), row0, n_snps,
                                         out.alt.data_ptr(), out.ref.data_ptr(), out.acnt.data_ptr(), out.rcnt.data_ptr(),
                                         _stream_ptr()), "ldx_bed_unpack_dev")

        if on_dev:
            if rows.device != dev:
                raise _lib.LdxError(f"from_bed: the rows are on {rows.device}, the panel on {dev}")
            if rows.stride(1) != 1:
                rows = rows.contiguous()
            for r0 in range(0, n_snps, chunk):
                unpack(rows[r0:r0 + chunk], r0)
        else:
            # two pinned buffers and two device buffers in turn: chunk k + 1 is copied in while chunk k unpacks
            width = int(rows.shape[1])
            pinned = [torch.empty((min(chunk, n_snps), width), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            staged = [torch.empty((min(chunk, n_snps), width), dtype=torch.uint8, device=dev) for _ in range(2)]
            done = [None, None]
            for k, r0 in enumerate(range(0, n_snps, chunk)):
                b, m = k & 1, min(chunk, n_snps - r0)
                if done[b] is not None:
                    done[b].synchronize()           # the copy out of this pinned buffer has finished
                np.copyto(pinned[b][:m].numpy(), rows[r0:r0 + m])
                staged[b][:m].copy_(pinned[b][:m], non_blocking=True)
                done[b] = torch.cuda.Event()
                done[b].record()
                unpack(staged[b][:m], r0)
        out.refresh_stats()
        return out

    def to_bed(self, alt: str = "a1", block_snps: int = 65536) -> np.ndarray:
        """The panel as PLINK SNP-major ``.bed`` rows, uint8 [n_snps][ceil(n_ind / 4)] on the host: ``plink.codes_bed_host`` of
        the panel's codes, byte for byte (include/ldx.h, ldx_bed_pack_dev) -- per individual both haplotypes ALT, both REF,
        one of each (a het, in either order), anything else a missing call.  Packed on the device and moved in blocks of
        ``block_snps`` rows."""
        from . import plink

        a2 = plink._alt_is_a2(alt)
        if self.n_hap % 2:
            raise _lib.LdxError(f"to_bed: n_hap={self.n_hap} is odd (individual k owns haplotypes 2k and 2k + 1)")
        nb = plink.row_bytes(self.n_ind)
        host = np.empty((self.n_snps, nb), dtype=np.uint8)
        block = max(1, min(int(block_snps), self.n_snps))
        buf = torch.empty((block, nb), dtype=torch.uint8, device=self.device)
        for r0 in range(0, self.n_snps, block):
            m = min(block, self.n_snps - r0)
            check(lib.ldx_bed_pack_dev(self.alt.data_ptr(), self.ref.data_ptr(), self.n_snps, self.n_hap, r0, m,
                                       buf.data_ptr(), nb, int(a2), _stream_ptr()), "ldx_bed_pack_dev")
            host[r0:r0 + m] = buf[:m].cpu().numpy()
        return host

    def pack_from(self, codes: torch.Tensor) -> None:
        """(Re)pack this panel from a device int8 matrix of its shape, on the current stream."""
        s = _stream_ptr()
        # one row has no row stride to speak of: numpy and torch report whatever the view's history left (codes[[i]][:, cols]
        # is a contiguous [1][n] matrix with stride 1), and the entry wants a leading dimension >= n_hap
        ld = codes.stride(0) if self.n_snps > 1 else max(codes.stride(0), self.n_hap)
        check(lib.ldx_pack_codes_dev(codes.data_ptr(), self.n_snps, self.n_hap, ld,
                                     self.alt.data_ptr(), self.ref.data_ptr(), self.acnt.data_ptr(),
                                     self.rcnt.data_ptr(), s), "ldx_pack_codes_dev")
        self.refresh_stats()

    def refresh_stats(self) -> None:
        check(lib.ldx_snp_stats_dev(self.acnt.data_ptr(), self.rcnt.data_ptr(), self.n_snps, self.n_hap,
                                    self.fa.data_ptr(), self.fr.data_ptr(), self.q.data_ptr(), _stream_ptr()),
              "ldx_snp_stats_dev")
        self.__dict__.pop("_dosage", None)   # the counts changed: dosage_stats() recomputes

    def dosage_stats(self):
        """``(hom, gstat)`` of include/ldx.h, ldx_dosage_stats_dev, on the device and cached until the panel is repacked:
        ``hom`` int32 [padded_snps] (bit pattern of uint32), the individuals with both alleles ALT, and ``gstat`` float64
        [padded_snps][2] = {a, 1 / sqrt(v)} with v = N (a + 2 hom) - a^2 (0 where v == 0): the per-SNP table of the dosage
        operators.  Individual k owns haplotypes 2k and 2k + 1, so ``n_hap`` must be even."""
        got = self.__dict__.get("_dosage")
        if got is None:
            if self.n_hap % 2:
                raise _lib.LdxError(f"dosage: n_hap={self.n_hap} is odd (individual k owns haplotypes 2k and 2k + 1)")
            npad = self.padded_snps
            hom = torch.empty(npad, dtype=torch.int32, device=self.device)
            gstat = torch.empty((npad, 2), dtype=torch.float64, device=self.device)
            check(lib.ldx_dosage_stats_dev(self.alt.data_ptr(), self.acnt.data_ptr(), self.n_snps, self.n_hap,
                                           hom.data_ptr(), gstat.data_ptr(), _stream_ptr()), "ldx_dosage_stats_dev")
            got = self.__dict__["_dosage"] = (hom, gstat)
        return got

    def dosage_live(self) -> np.ndarray:
        """bool [n_snps]: the SNPs whose dosage has variance among the individuals (v > 0)."""
        return self.dosage_stats()[1][: self.n_snps, 1].cpu().numpy() > 0.0

    # ------------------------------------------------------------------ subsets
    def select(self, snps=None, haplotypes=None, out: Optional["PackedPanel"] = None) -> "PackedPanel":
        """The panel of the chosen SNPs and / or haplotypes of this one (include/ldx.h, ldx_panel_select_dev): row i,
        haplotype h of the result is row snps[i], haplotype haplotypes[h] of this panel -- what ``from_codes`` makes of
        ``codes[snps][:, haplotypes]``, byte for byte, straight from the bit planes on the current stream.  Each argument is
        an integer index array (numpy, list or torch, host or device; any order, repeats allowed: a bootstrap) or a boolean
        mask of the source length; None keeps the axis.  ``out``: a panel of the result's shape to write into (every byte of
        it is written).  Indices are checked on the host first: out-of-range and negative ones raise LdxError."""
        require_gpu()
        if snps is None and haplotypes is None:
            raise _lib.LdxError("select: give snps, haplotypes or both")
        si = None if snps is None else select_index(snps, self.n_snps, "SNP")
        hi = None if haplotypes is None else select_index(haplotypes, self.n_hap, "haplotype")
        n_snps = self.n_snps if si is None else int(si.size)
        n_hap = self.n_hap if hi is None else int(hi.size)
        if n_hap > _lib.MAX_HAPS:
            raise _lib.LdxError(f"select: {n_hap} haplotypes selected, more than {_lib.MAX_HAPS} (LDX_MAX_HAPS)")
        if out is None:
            dev = self.device
            pb, npad = lib.ldx_plane_bytes(n_snps, n_hap), lib.ldx_padded_snps(n_snps)
            e = lambda n, dt: torch.empty(n, dtype=dt, device=dev)  # noqa: E731  (the call writes every byte)
            out = PackedPanel(n_snps, n_hap, e(pb, torch.uint8), e(pb, torch.uint8), e(npad, torch.int32),
                              e(npad, torch.int32), e(npad, torch.float64), e(npad, torch.float64), e(npad, torch.float64))
        elif out is self:
            raise _lib.LdxError("select: out must not be the source panel")
        elif (out.n_snps, out.n_hap) != (n_snps, n_hap) or out.device != self.device:
            raise _lib.LdxError(f"select: out is a {out.n_snps} x {out.n_hap} panel on {out.device}, "
                                f"the selection is {n_snps} x {n_hap} on {self.device}")
        to_dev = lambda a: None if a is None else torch.from_numpy(a.view(np.int32)).to(self.device)  # noqa: E731
        sd, hd = to_dev(si), to_dev(hi)
        check(lib.ldx_panel_select_dev(self.alt.data_ptr(), self.ref.data_ptr(), self.n_snps, self.n_hap,
                                       _ptr(sd), n_snps, _ptr(hd), n_hap, out.alt.data_ptr(), out.ref.data_ptr(),
                                       out.acnt.data_ptr(), out.rcnt.data_ptr(), _stream_ptr()), "ldx_panel_select_dev")
        out.refresh_stats()
        return out

    def split(self, labels) -> dict:
        """``{label: the panel of that label's haplotypes, in source order}`` for one hashable label per haplotype (a
        population or gender per haplotype: the reference's -e / -g choice, answered for every value at once)."""
        labels = list(labels)
        if len(labels) != self.n_hap:
            raise _lib.LdxError(f"split: {len(labels)} labels for {self.n_hap} haplotypes")
        columns: dict = {}
        for h, label in enumerate(labels):
            columns.setdefault(label, []).append(h)
        return {label: self.select(haplotypes=np.asarray(cols, dtype=np.uint32)) for label, cols in columns.items()}

    # ------------------------------------------------------------------ geometry
    @property
    def padded_snps(self) -> int:
        return lib.ldx_padded_snps(self.n_snps)

    @property
    def n_ind(self) -> int:
        """Individuals of the dosage operators: n_hap // 2 (haplotypes 2k and 2k + 1 belong to individual k)."""
        return self.n_hap // 2

    @property
    def n_pairs(self) -> int:
        return self.n_snps * (self.n_snps - 1) // 2

    @property
    def n_units(self) -> int:
        return lib.ldx_triangle_units(self.n_snps)

    @property
    def device(self) -> torch.device:
        return self.alt.device

    # ------------------------------------------------------------------ per-SNP results
    def alt_counts(self) -> np.ndarray:
        return self.acnt[: self.n_snps].cpu().numpy().view(np.uint32)

    def ref_counts(self) -> np.ndarray:
        return self.rcnt[: self.n_snps].cpu().numpy().view(np.uint32)

    def alt_freq4(self) -> torch.Tensor:
        """round(a/n, 4) per SNP (calc_ld.py:96-97, ld_area.py:188-189), float64 on device."""
        out = torch.empty(self.n_snps, dtype=torch.float64, device=self.device)
        check(lib.ldx_alt_freq4_dev(self.acnt.data_ptr(), self.n_snps, self.n_hap, out.data_ptr(),
                                    _stream_ptr()), "ldx_alt_freq4_dev")
        return out

    def clear_area_plans(self) -> None:
        """Drop the ld_area plans kept on this panel (ops.ld_area: buffers + HIP graph per call shape) and their memory."""
        self.__dict__.pop("_area_plans", None)
