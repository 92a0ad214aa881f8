"""PLINK 1 binary filesets (.bed / .bim / .fam) on the host: the file semantics, stated once.  Pure numpy; the device
kernels (include/ldx.h, ldx_bed_unpack_dev / ldx_bed_pack_dev) are tested against the two converters of this module.

A SNP-major ``.bed`` holds, after the three magic bytes ``6c 1b 01``, one row of ceil(n_ind / 4) bytes per variant.
Individual k is the 2-bit field at bits 2 (k % 4), 2 (k % 4) + 1 of byte k // 4, low bit first:

    00  homozygous A1        01 (low bit set, high bit clear)  missing        10  heterozygous        11  homozygous A2

A packed panel holds individual k as haplotypes 2k and 2k + 1.  With ``alt="a1"`` (PLINK and LDSC count A1) the codes are
hom A1 -> (1, 1), het -> (1, 0), hom A2 -> (0, 0), missing -> (2, 2); a het always puts the ALT allele on haplotype 2k: a
``.bed`` carries no phase.  ``alt="a2"`` swaps the two homozygotes and leaves the het.  Bits past n_ind in a row's last byte
are ignored on reading and written as zero.
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence

import numpy as np

from ._lib import LdxError

MAGIC = bytes((0x6C, 0x1B, 0x01))
ALTS = ("a1", "a2")


def row_bytes(n_ind: int) -> int:
    """Bytes of one SNP-major row: ceil(n_ind / 4)."""
    return (int(n_ind) + 3) // 4


def _alt_is_a2(alt: str) -> bool:
    if alt not in ALTS:
        raise LdxError(f"alt must be 'a1' or 'a2' (got {alt!r})")
    return alt == "a2"


def _keep_index(keep, n_ind: int) -> Optional[np.ndarray]:
    if keep is None:
        return None
    from .panel import select_index   # (torch only where the panel module needs it)

    return select_index(keep, n_ind, "individual")


def _rows(rows_u8, n_ind: int) -> np.ndarray:
    rows = np.asarray(rows_u8)
    if rows.dtype != np.uint8 or rows.ndim != 2:
        raise LdxError("bed rows must be a uint8 matrix [n_snps][ceil(n_ind / 4)]")
    if n_ind < 1 or rows.shape[1] < row_bytes(n_ind):
        raise LdxError(f"bed rows of {rows.shape[1]} bytes cannot hold {n_ind} individuals")
    return rows


def bed_fields_host(rows_u8, n_ind: int) -> np.ndarray:
    """uint8 [n_snps][n_ind]: the 2-bit field of every individual (0 hom A1, 1 missing, 2 het, 3 hom A2)."""
    rows = _rows(rows_u8, n_ind)[:, : row_bytes(n_ind)]
    f = (rows[:, :, None] >> np.array([0, 2, 4, 6], dtype=np.uint8)) & np.uint8(3)
    return f.reshape(rows.shape[0], -1)[:, :n_ind]


def bed_codes_host(rows_u8, n_ind: int, keep=None, alt: str = "a1") -> np.ndarray:
    """int8 [n_snps][2 * n_kept] allele codes of SNP-major ``.bed`` rows (the module docstring's table).  ``keep``: an index
    array over the file's individuals (any order, repeats allowed) or a boolean mask, with ``panel.select_index``'s rules."""
    a2 = _alt_is_a2(alt)
    f = bed_fields_host(rows_u8, n_ind)
    idx = _keep_index(keep, n_ind)
    if idx is not None:
        f = f[:, idx]
    # field -> (code of haplotype 2k, code of haplotype 2k + 1)
    first = np.array([0, 2, 1, 1] if a2 else [1, 2, 1, 0], dtype=np.int8)
    second = np.array([0, 2, 0, 1] if a2 else [1, 2, 0, 0], dtype=np.int8)
    out = np.empty((f.shape[0], 2 * f.shape[1]), dtype=np.int8)
    out[:, 0::2] = first[f]
    out[:, 1::2] = second[f]
    return out


def codes_bed_host(codes, alt: str = "a1") -> np.ndarray:
    """uint8 [n_snps][ceil(n_ind / 4)]: the ``.bed`` rows of an int8 [n_snps][2 * n_ind] code matrix, the inverse of
    ``bed_codes_host``.  Per individual: both codes ALT (1) -> hom ALT, both REF (0) -> hom REF, one of each in either order ->
    het, anything else (any other code) -> missing.  Pad bits are zero."""
    a2 = _alt_is_a2(alt)
    c = np.asarray(codes)
    if c.ndim != 2 or c.shape[1] % 2 or c.shape[1] == 0:
        raise LdxError("codes must be a matrix [n_snps][2 * n_ind]")
    x, y = c[:, 0::2], c[:, 1::2]
    hom_alt = (x == 1) & (y == 1)
    hom_ref = (x == 0) & (y == 0)
    het = ((x == 1) & (y == 0)) | ((x == 0) & (y == 1))
    f = np.full(x.shape, 1, dtype=np.uint8)
    f[hom_alt] = 3 if a2 else 0
    f[hom_ref] = 0 if a2 else 3
    f[het] = 2
    n_ind = x.shape[1]
    pad = np.zeros((f.shape[0], 4 * row_bytes(n_ind)), dtype=np.uint8)
    pad[:, :n_ind] = f
    q = pad.reshape(f.shape[0], -1, 4)
    return (q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8)


def canonical_codes(codes) -> np.ndarray:
    """What ``bed_codes_host(codes_bed_host(codes))`` returns: per individual (1, 1), (0, 0), (1, 0) for a het in either
    order, (2, 2) for anything else."""
    c = np.asarray(codes)
    x, y = c[:, 0::2], c[:, 1::2]
    het = ((x == 1) & (y == 0)) | ((x == 0) & (y == 1))
    same = (x == y) & ((x == 0) | (x == 1))
    out = np.full(c.shape, 2, dtype=np.int8)
    out[:, 0::2] = np.where(same, x, np.where(het, 1, 2))
    out[:, 1::2] = np.where(same, y, np.where(het, 0, 2))
    return out


def _prefix(path) -> str:
    p = os.fspath(path)
    return p[:-4] if p.endswith(".bed") else p


def _read_table(path: str, n_fields: int, what: str) -> List[List[str]]:
    rows = []
    try:
        with open(path) as f:
            for ln, line in enumerate(f, 1):
                parts = line.split()
                if not parts:
                    continue
                if len(parts) != n_fields:
                    raise LdxError(f"{path}:{ln}: {len(parts)} fields, a {what} line has {n_fields}")
                rows.append(parts)
    except OSError as exc:
        raise LdxError(f"cannot read {path}: {exc}") from exc
    if not rows:
        raise LdxError(f"{path}: no {what} lines")
    return rows


def _numbers(col: Sequence[str], kind, path: str, name: str) -> np.ndarray:
    try:
        return np.asarray([kind(v) for v in col])
    except ValueError as exc:
        raise LdxError(f"{path}: column {name} is not numeric ({exc})") from exc


class BedFile:
    """An open SNP-major fileset.  ``chrom``, ``ids``, ``a1``, ``a2`` (lists of str), ``cm`` (float64), ``pos`` (int64) from
    ``.bim``; ``fid``, ``iid``, ``father``, ``mother``, ``sex``, ``pheno`` (lists of str) from ``.fam``; ``rows``: the
    genotype rows as a read-only ``np.memmap`` uint8 [n_snps][ceil(n_ind / 4)].  Every malformed input raises LdxError."""

    def __init__(self, prefix):
        self.prefix = _prefix(prefix)
        bim = _read_table(self.prefix + ".bim", 6, ".bim")
        fam = _read_table(self.prefix + ".fam", 6, ".fam")
        self.chrom = [r[0] for r in bim]
        self.ids = [r[1] for r in bim]
        self.cm = _numbers([r[2] for r in bim], float, self.prefix + ".bim", "cM").astype(np.float64)
        self.pos = _numbers([r[3] for r in bim], int, self.prefix + ".bim", "position").astype(np.int64)
        self.a1 = [r[4] for r in bim]
        self.a2 = [r[5] for r in bim]
        self.fid, self.iid, self.father, self.mother, self.sex, self.pheno = ([r[k] for r in fam] for k in range(6))
        self.n_snps, self.n_ind = len(bim), len(fam)
        path = self.prefix + ".bed"
        try:
            size = os.path.getsize(path)
            with open(path, "rb") as f:
                magic = f.read(3)
        except OSError as exc:
            raise LdxError(f"cannot read {path}: {exc}") from exc
        if len(magic) < 3 or magic[:2] != MAGIC[:2]:
            raise LdxError(f"{path}: not a PLINK .bed file (magic bytes {magic.hex()})")
        if magic[2] == 0:
            raise LdxError(f"{path}: an individual-major .bed (third byte 00); only SNP-major files are read")
        if magic[2] != 1:
            raise LdxError(f"{path}: not a PLINK .bed file (magic bytes {magic.hex()})")
        want = 3 + self.n_snps * row_bytes(self.n_ind)
        if size != want:
            raise LdxError(f"{path}: {size} bytes, but {self.n_snps} variants (.bim) x {self.n_ind} individuals (.fam) need "
                           f"{want}")
        self.rows = np.memmap(path, dtype=np.uint8, mode="r", offset=3, shape=(self.n_snps, row_bytes(self.n_ind)))

    def bim(self, snps=None) -> dict:
        """The .bim columns (of the variants ``snps``, an index array) as write_bfile takes them."""
        k = range(self.n_snps) if snps is None else [int(i) for i in snps]
        return {"chrom": [self.chrom[i] for i in k], "ids": [self.ids[i] for i in k], "cm": self.cm[list(k)],
                "pos": self.pos[list(k)], "a1": [self.a1[i] for i in k], "a2": [self.a2[i] for i in k]}

    def fam(self, individuals=None) -> dict:
        """The .fam columns (of the individuals ``individuals``, an index array) as write_bfile takes them."""
        k = range(self.n_ind) if individuals is None else [int(i) for i in individuals]
        return {name: [getattr(self, name)[i] for i in k] for name in ("fid", "iid", "father", "mother", "sex", "pheno")}


def _column(table: dict, name: str, n: Optional[int], default=None) -> list:
    col = table.get(name)
    if col is None:
        if default is None:
            raise LdxError(f"write_bfile: column {name!r} is missing")
        col = [default] * n
    return list(col)


def _fmt_cm(v) -> str:
    v = float(v)
    return str(int(v)) if v == int(v) else repr(v)


def write_bfile(prefix, rows_u8, bim: dict, fam: dict) -> List[str]:
    """Write ``prefix.bed`` / ``.bim`` / ``.fam``.  ``rows_u8``: uint8 [n_snps][ceil(n_ind / 4)]; ``bim``: chrom, ids, pos, a1,
    a2 and optionally cm (default 0), one entry per variant; ``fam``: iid and optionally fid (default: iid), father, mother,
    sex (default 0) and pheno (default -9), one entry per individual.  Returns the three paths."""
    prefix = _prefix(prefix)
    iid = _column(fam, "iid", None)
    n_ind = len(iid)
    ids = _column(bim, "ids", None)
    n_snps = len(ids)
    rows = np.asarray(rows_u8)
    if rows.dtype != np.uint8 or rows.shape != (n_snps, row_bytes(n_ind)):
        raise LdxError(f"write_bfile: rows of shape {rows.shape} ({rows.dtype}) for {n_snps} variants x {n_ind} individuals")
    bim_cols = [_column(bim, "chrom", n_snps), ids, [_fmt_cm(v) for v in _column(bim, "cm", n_snps, 0)],
                [str(int(v)) for v in _column(bim, "pos", n_snps)], _column(bim, "a1", n_snps), _column(bim, "a2", n_snps)]
    fam_cols = [list(fam["fid"]) if fam.get("fid") is not None else iid, iid,
                _column(fam, "father", n_ind, "0"), _column(fam, "mother", n_ind, "0"), _column(fam, "sex", n_ind, "0"),
                _column(fam, "pheno", n_ind, "-9")]
    for cols, n, what in ((bim_cols, n_snps, "bim"), (fam_cols, n_ind, "fam")):
        if any(len(c) != n for c in cols):
            raise LdxError(f"write_bfile: the {what} columns differ in length")
    paths = [prefix + ".bed", prefix + ".bim", prefix + ".fam"]
    with open(paths[0], "wb") as f:
        f.write(MAGIC)
        f.write(np.ascontiguousarray(rows).tobytes())
    with open(paths[1], "w") as f:
        f.writelines("\t".join(str(c[k]) for c in bim_cols) + "\n" for k in range(n_snps))
    with open(paths[2], "w") as f:
        f.writelines(" ".join(str(c[k]) for c in fam_cols) + "\n" for k in range(n_ind))
    return paths


# ---------------------------------------------------------------------------------------------- phenotype and covariate tables
PHENO_MISSING = ("NA", "nan", "-9")


def _sample_table(path: str, what: str, missing: Sequence[str]):
    """(fid, iid, names, values float64 [lines, len(names)]) of a whitespace table whose header is ``#FID IID ...``,
    ``FID IID ...`` or ``#IID ...`` (``fid`` is None then: the table names its individuals by IID alone); a field in ``missing``
    reads as NaN.  An individual named on two lines is refused."""
    try:
        with open(path) as f:
            lines = [ln.split() for ln in f if ln.split()]
    except OSError as exc:
        raise LdxError(f"cannot read {path}: {exc}") from exc
    if not lines:
        raise LdxError(f"{path}: empty {what} table")
    head = lines[0]
    if head[0] in ("#FID", "FID") and len(head) >= 2 and head[1] == "IID":
        n_id = 2
    elif head[0] in ("#IID", "IID"):
        n_id = 1
    else:
        raise LdxError(f"{path}: the header of a {what} table starts with '#FID IID', 'FID IID' or '#IID', not {head[0]!r}")
    names = head[n_id:]
    if not names:
        raise LdxError(f"{path}: no {what} column")
    if len(set(names)) != len(names):
        raise LdxError(f"{path}: a {what} name is repeated")
    fid, iid, rows, seen = [], [], [], set()
    for no, parts in enumerate(lines[1:], 2):
        if len(parts) != len(head):
            raise LdxError(f"{path}: line {no}: {len(parts)} fields beside the header's {len(head)}")
        iid.append(parts[n_id - 1])
        fid.append(parts[0])
        key = (fid[-1], iid[-1])
        if key in seen:
            raise LdxError(f"{path}: line {no}: individual {' '.join(key[2 - n_id:])} has a line already")
        seen.add(key)
        try:
            rows.append([float("nan") if v in missing else float(v) for v in parts[n_id:]])
        except ValueError:
            raise LdxError(f"{path}: line {no}: a {what} value that is no number") from None
    return (fid if n_id == 2 else None), iid, names, np.asarray(rows, dtype=np.float64).reshape(len(rows), len(names))


def read_pheno(path) -> tuple:
    """(fid, iid, names, values) of a phenotype table (PLINK 2's --pheno): ``NA``, ``nan`` and ``-9`` are missing (NaN);
    ``fid`` is None when the table has no FID column."""
    return _sample_table(os.fspath(path), "phenotype", PHENO_MISSING)


def read_covar(path) -> tuple:
    """(fid, iid, names, values) of a covariate table (PLINK 2's --covar; an ``.eigenvec`` is one): ``NA`` and ``nan`` are
    missing (NaN); -9 is a value."""
    return _sample_table(os.fspath(path), "covariate", PHENO_MISSING[:2])
