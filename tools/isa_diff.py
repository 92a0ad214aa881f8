#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two versions of the library, kernel by kernel.  CPU only: it compiles to
assembly and reads text, it loads no library and needs no GPU.

    python tools/isa_diff.py BEFORE AFTER [--keep DIR] [--text ldx_mfma.hip ...]

BEFORE and AFTER are each a source tree (a checkout: its ld_tools_amd/build.py names the sources and the flags) or a
directory of `.s` files made earlier (--keep writes them, as DIR/before and DIR/after).  Every file of build.SOURCES is
compiled with build.FLAGS (without -shared) plus `--cuda-device-only -S`.  Of each function the instructions are kept --
comments, directives, labels and the per-compile __hip_cuid_* symbol are dropped -- and per function the tool prints
    text       whether the instruction text is identical,
    mnemonics  whether the sequence of first tokens is identical (register numbering and operand order may then differ),
and, for kernels, .vgpr_count / .sgpr_count / .private_segment_fixed_size / .group_segment_fixed_size on both sides.

Exit status 1 if a function exists on one side only, a mnemonic sequence or a resource figure differs, or the text differs
in a file named with --text; 0 otherwise.  A refactor that claims "same code" shows this tool's output.
"""
from __future__ import annotations

import argparse
import importlib.util
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

FIGURES = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")
LABEL = re.compile(r"^([A-Za-z_$.][\w$.]*):")
NEW_KERNEL = re.compile(r"^  - \.(\w+):\s*(.*)$")
KERNEL_KEY = re.compile(r"^    \.(\w+):\s*(.*)$")


def load_build(tree: Path):
    spec = importlib.util.spec_from_file_location(f"ldx_build_{abs(hash(str(tree)))}", tree / "ld_tools_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_tree(tree: Path, out: Path) -> None:
    """one hipcc per source of the tree's build.SOURCES, side by side, each to out/<stem>.s"""
    b = load_build(tree)
    out.mkdir(parents=True, exist_ok=True)
    flags = [f for f in b.FLAGS if f != "-shared"] + ["--cuda-device-only", "-S"]
    cmds = [[b.hipcc(), *flags, str(b.CSRC / s), "-o", str(out / (Path(s).stem + ".s"))] for s in b.SOURCES]

    def run(c):
        return subprocess.run(c, capture_output=True, text=True)

    with ThreadPoolExecutor(max_workers=len(cmds)) as pool:
        for c, r in zip(cmds, pool.map(run, cmds)):
            if r.returncode != 0:
                raise SystemExit(f"hipcc failed ({r.returncode}): {' '.join(c)}\n{r.stderr}")


def parse(path: Path):
    """-> ({function: [instruction, ...]}, {kernel: {figure: value}}), functions in file order"""
    funcs: dict[str, list[str]] = {}
    figures: dict[str, dict[str, str]] = {}
    types = set()
    cur = None          # the function whose body is being read
    entry = None        # the metadata record being read
    in_meta = False
    for raw in path.read_text().splitlines():
        if raw.startswith("\t.type\t") and raw.endswith(",@function"):
            types.add(raw.split("\t")[2].split(",")[0])
        if raw.startswith("\t.amdgpu_metadata") or raw.startswith(".amdgpu_metadata"):
            in_meta = True
            continue
        if in_meta:
            m = NEW_KERNEL.match(raw)
            if m:
                entry = {}
            m = m or KERNEL_KEY.match(raw)
            if m and entry is not None:
                entry[m.group(1)] = m.group(2).strip().strip("'\"")
                if m.group(1) == "vgpr_count":      # the last key of a record (they are sorted)
                    figures[entry["name"]] = {k: entry.get(k, "?") for k in FIGURES}
            continue
        m = LABEL.match(raw)
        if m:
            name = m.group(1)
            if name in types:
                cur = funcs.setdefault(name, [])
            elif name.startswith(".Lfunc_end"):
                cur = None
            continue
        if cur is None:
            continue
        line = raw.split(";", 1)[0].strip()
        if not line or line.startswith(".") or "__hip_cuid_" in line:
            continue
        cur.append(" ".join(line.split()))
    return funcs, figures


def demangled(names):
    if not names:
        return {}
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, map(short, r.stdout.splitlines())))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def short(name: str) -> str:
    """a demangled name without its parameter list (the template arguments stay: they tell the instantiations apart)"""
    depth = 0
    for k, ch in enumerate(name):
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            return name[:k].removeprefix("void ")
    return name


def side(arg: str, keep: Path | None, label: str, tmp: Path) -> Path:
    p = Path(arg).resolve()
    if (p / "ld_tools_amd" / "build.py").exists():
        out = (keep or tmp) / label
        compile_tree(p, out)
        return out
    if not list(p.glob("*.s")):
        raise SystemExit(f"{arg}: neither a source tree nor a directory of .s files")
    return p


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--keep", type=Path, help="write the .s files of compiled trees to DIR/before and DIR/after")
    ap.add_argument("--text", nargs="*", default=[], metavar="SOURCE",
                    help="sources whose functions must have identical text, not only identical mnemonics")
    a = ap.parse_args()
    strict = {Path(s).stem for s in a.text}
    bad = 0
    with tempfile.TemporaryDirectory() as t:
        with ThreadPoolExecutor(max_workers=2) as pool:
            d0, d1 = pool.map(lambda x: side(x[0], a.keep, x[1], Path(t)), [(a.before, "before"), (a.after, "after")])
        stems = sorted({f.stem for f in d0.glob("*.s")} | {f.stem for f in d1.glob("*.s")})
        for stem in stems:
            f0, f1 = d0 / f"{stem}.s", d1 / f"{stem}.s"
            if not (f0.exists() and f1.exists()):
                print(f"== {stem}: only {'before' if f0.exists() else 'after'}")
                bad += 1
                continue
            (fn0, fig0), (fn1, fig1) = parse(f0), parse(f1)
            names = list(fn0) + [n for n in fn1 if n not in fn0]
            pretty = demangled(names)
            print(f"== {stem}: {len(names)} functions" + ("   (identical text required)" if stem in strict else ""))
            for n in names:
                if n not in fn0 or n not in fn1:
                    print(f"  ONLY {'before' if n in fn0 else 'after '}  {pretty[n]}")
                    bad += 1
                    continue
                i0, i1 = fn0[n], fn1[n]
                text = i0 == i1
                mnem = [x.split()[0] for x in i0] == [x.split()[0] for x in i1]
                g0, g1 = fig0.get(n), fig1.get(n)
                figs = ""
                if g0 or g1:
                    g0, g1 = g0 or {}, g1 or {}
                    figs = "  " + " ".join(f"{k.split('_')[0]} {g0.get(k, '?')}/{g1.get(k, '?')}" for k in FIGURES)
                same_figs = g0 == g1
                if not mnem or not same_figs or (stem in strict and not text):
                    bad += 1
                print(f"  text {'same' if text else 'DIFF'}  mnemonics {'same' if mnem else 'DIFF'}  "
                      f"instr {len(i0)}/{len(i1)}{figs}{'' if same_figs else '  FIGURES DIFFER'}  {pretty[n]}")
    print(f"== {'all required comparisons hold' if not bad else f'{bad} function(s) miss a required comparison'}"
          "   (figures: vgpr sgpr private(scratch) group(LDS), before/after)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
