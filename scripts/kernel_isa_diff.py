#!/usr/bin/env python3
"""Is the gfx950 machine code of every kernel of a translation unit unchanged by a source edit?

Compiles csrc/kernels/<file> of two source trees -- OLD (default: the csrc of git HEAD) and NEW
(default: the working tree's csrc) -- device-only to assembly with the build's own flags
(--offload-arch=gfx950 --cuda-device-only -S -O3 -std=c++17 -I <csrc>/include), streams each
output kernel by kernel (nothing but one running hash per kernel is kept: conv_fwd.hip is ~1.1 M
lines), normalises the kernel's own symbol and the function-numbered labels, and compares per
kernel a digest over its instruction stream, local labels and .amdhsa_* descriptor directives.

Kernels are matched old to new by name and decoded integer template arguments; LEGACY maps the
positional-bool template signatures of the LDS-DMA forward kernels before the flags refactor to
today's <BP, BC, WAVES_P, NS, NW, BK, NH, F>. Kernels present on one side only are listed. The
report has one line per kernel: name, instruction count, old and new digest, and the compiler's
resource remarks (scripts/kernel_resources.py): VGPRs, AGPRs, occupancy, spill, scratch, LDS.

    python scripts/kernel_isa_diff.py conv_fwd.hip [--old DIR] [--new DIR] [--work DIR] [--reuse]
                                      [--strip-iso] [--out report.txt]

--strip-iso: OLD is a copy of NEW with every `#if(n)def DRN_ISO_*` block resolved as undefined,
i.e. the check that the bound-isolation hooks, compiled out, add nothing to the default build.
Exit status 0 only if the kernel sets match one-to-one and every digest is equal.
"""
import argparse
import hashlib
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "scripts"))
from kernel_resources import REMARKS, parse_remarks  # noqa: E402

K_PF, K_PRO, K_SROW, K_KS, K_IL = 1, 2, 4, 8, 16


def _legacy_glds(a):  # <BP, BC, WAVES_P, NS, NW, PF, BK, PRO, SROW, NH, KS, IL>
    bp, bc, wp, ns, nw, pf, bk, pro, srow, nh, ks, il = a
    return (bp, bc, wp, ns, nw, bk, nh, pf * K_PF | pro * K_PRO | srow * K_SROW | ks * K_KS | il * K_IL)


def _legacy_glds_sk(a):  # <BP, BC, WAVES_P, NS, NW, BK, PRO, NH, IL>
    bp, bc, wp, ns, nw, bk, pro, nh, il = a
    return (bp, bc, wp, ns, nw, bk, nh, K_KS | pro * K_PRO | il * K_IL)


# kernel name -> (template arity of the old signature, map to today's arguments)
LEGACY = {"conv_fwd_glds_kernel": (12, _legacy_glds), "conv_fwd_glds_sk_kernel": (9, _legacy_glds_sk)}


def kernel_key(mangled: str):
    """(name, integer template arguments) of drn::name<ints...>(...); the mangled name itself
    for anything else (then old and new must agree on it)."""
    m = re.match(r"_ZN3drn(\d+)", mangled)
    if not m:
        return (mangled, ())
    n = int(m.group(1))
    name, rest = mangled[m.end():m.end() + n], mangled[m.end() + n:]
    if not rest.startswith("I"):
        return (mangled, ())
    args, pos = [], 1
    while True:
        t = re.match(r"L[a-z](n?)(\d+)E", rest[pos:])
        if not t:
            break
        args.append(-int(t.group(2)) if t.group(1) else int(t.group(2)))
        pos += t.end()
    if not rest[pos:].startswith("E"):  # a non-integer template argument
        return (mangled, ())
    if name in LEGACY and len(args) == LEGACY[name][0]:
        args = LEGACY[name][1](args)
    return (name, tuple(args))


def compile_asm(csrc: Path, fname: str, out: Path, reuse: bool):
    asm, err = out / (Path(fname).stem + ".s"), out / (Path(fname).stem + ".err")
    if reuse and asm.exists() and err.exists():
        return asm, err
    out.mkdir(parents=True, exist_ok=True)
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-O3", "-std=c++17",
           "-I", str(csrc / "include"), REMARKS, str(csrc / "kernels" / fname), "-o", str(asm)]
    with open(err, "w") as e:
        rc = subprocess.run(cmd, stderr=e).returncode
    if rc != 0:
        sys.exit(f"hipcc failed for {csrc / 'kernels' / fname}: see {err}")
    return asm, err


def kernel_digests(asm: Path) -> dict:
    """{mangled name: (instructions, digest)}, streaming the assembly file."""
    out = {}
    name = h = None
    n = 0
    with open(asm, errors="replace") as f:
        for line in f:
            if name is None:
                m = re.match(r"(\S+):\s+; @(\S+)", line)
                if m and m.group(1) == m.group(2):
                    name, h, n = m.group(1), hashlib.sha256(), 0
                continue
            s = line.split(";", 1)[0].strip()
            if s.startswith(".end_amdhsa_kernel"):
                out[name] = (n, h.hexdigest()[:16])
                name = None
                continue
            if not s:
                continue
            if s.startswith("."):
                if not (s.startswith(".amdhsa_") and not s.startswith(".amdhsa_kernel")) and \
                        not re.match(r"\.LBB\d+_\d+:", s):
                    continue  # sections, alignment, .amdhsa_kernel <name>
            else:
                n += 1
            s = s.replace(name, "@self")
            s = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", s)
            h.update(s.encode() + b"\n")
    return out


def strip_iso(src: Path, dst: Path):
    """Copy csrc to dst with every #ifdef / #ifndef DRN_ISO_* block resolved as undefined."""
    shutil.copytree(src, dst)
    for p in list((dst / "kernels").glob("*.hip")) + list((dst / "include").glob("*.h")):
        keep, stack = [], []  # stack: per open conditional, None (not ours) or [emitting?]
        for line in p.read_text().splitlines(keepends=True):
            t = line.strip()
            m = re.match(r"#\s*(ifdef|ifndef)\s+DRN_ISO_\w+", t)
            if m:
                stack.append([m.group(1) == "ifndef"])
                continue
            if re.match(r"#\s*if", t):
                stack.append(None)
            elif re.match(r"#\s*else", t) and stack and stack[-1] is not None:
                stack[-1][0] = not stack[-1][0]
                continue
            elif re.match(r"#\s*endif", t):
                if stack.pop() is not None:
                    continue
            if all(s is None or s[0] for s in stack):
                keep.append(line)
        p.write_text("".join(keep))


def fmt_res(r):
    return " ".join(f"{k}={r.get(v)}" for k, v in (("vgpr", "VGPRs"), ("agpr", "AGPRs"), ("occ", "Occupancy"),
                                                    ("spill", "VGPRs_spill"), ("scratch", "ScratchSize"),
                                                    ("lds", "LDS")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("file", help="translation unit under csrc/kernels, e.g. conv_fwd.hip")
    ap.add_argument("--old", default="", help="old csrc directory (default: csrc of git HEAD)")
    ap.add_argument("--new", default=str(ROOT / "csrc"))
    ap.add_argument("--work", default="", help="directory for the assembly (default: a temporary one)")
    ap.add_argument("--reuse", action="store_true", help="reuse assembly already in --work")
    ap.add_argument("--strip-iso", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    tmp = Path(tempfile.mkdtemp(prefix="drn_isa_"))
    work = Path(a.work) if a.work else tmp
    new = Path(a.new)
    if a.strip_iso:
        old, what = tmp / "stripped", "NEW with the DRN_ISO_* blocks removed"
        strip_iso(new, old)
    elif a.old:
        old, what = Path(a.old), a.old
    else:
        old, what = tmp / "head" / "csrc", "git HEAD"
        (tmp / "head").mkdir()
        tar = subprocess.run(["git", "-C", str(ROOT), "archive", "HEAD", "csrc"], capture_output=True, check=True)
        subprocess.run(["tar", "-x", "-C", str(tmp / "head")], input=tar.stdout, check=True)
    sides = {}
    for tag, csrc in (("old", old), ("new", new)):
        asm, err = compile_asm(csrc, a.file, work / tag, a.reuse)
        dig = kernel_digests(asm)
        with open(err, errors="replace") as f:
            res = parse_remarks(f)
        sides[tag] = {kernel_key(k): (k, n, d, res.get(k, {})) for k, (n, d) in dig.items()}
        if len(sides[tag]) != len(dig):
            sys.exit(f"{tag}: two kernels decode to the same key")
    o, n = sides["old"], sides["new"]
    both = sorted(set(o) & set(n))
    only_o, only_n = sorted(set(o) - set(n)), sorted(set(n) - set(o))
    differ = [k for k in both if o[k][1:3] != n[k][1:3]]
    res_differ = [k for k in both if o[k][3] != n[k][3]]
    lines = [f"# {a.file}: OLD = {what}, NEW = {'working tree' if new == ROOT / 'csrc' else new}",
             f"# kernels old {len(o)} new {len(n)} matched {len(both)}; only old {len(only_o)}, only new {len(only_n)}; "
             f"streams identical {len(both) - len(differ)}, different {len(differ)}; resources different {len(res_differ)}",
             "# kernel | instructions | old digest | new digest | resources (old -> new when different)"]
    for k in both:
        r = fmt_res(n[k][3]) if o[k][3] == n[k][3] else f"{fmt_res(o[k][3])} -> {fmt_res(n[k][3])}"
        flag = "" if k not in differ else f"  DIFFERENT (old {o[k][1]} instructions)"
        lines.append(f"{n[k][0]} | {n[k][1]} | {o[k][2]} | {n[k][2]} | {r}{flag}")
    lines += [f"ONLY OLD {o[k][0]} | {o[k][1]} | {o[k][2]}" for k in only_o]
    lines += [f"ONLY NEW {n[k][0]} | {n[k][1]} | {n[k][2]}" for k in only_n]
    text = "\n".join(lines) + "\n"
    if a.out:
        Path(a.out).write_text(text)
    print("\n".join(lines[:2] + [ln for ln in lines[3:] if "DIFFERENT" in ln or ln.startswith("ONLY")][:40]))
    shutil.rmtree(tmp, ignore_errors=True)
    sys.exit(1 if differ or only_o or only_n or res_differ else 0)


if __name__ == "__main__":
    main()
