"""Machine-code check for a refactor of the native kernels: did any kernel's gfx950 code change?

``dump`` (run once per checkout) compiles every ``.hip`` of ``build.KERNEL_SOURCES`` with the build's own flags
plus ``--offload-device-only -S`` and records, per kernel, its register / scratch / LDS footprint, its instruction
count and a hash of its normalised instruction stream (comments and directives stripped, local labels renumbered
in order of appearance, mangled symbol names replaced by a placeholder).  ``compare`` matches the kernels of two
dumps by demangled name with namespaces stripped and reports which are identical and how the rest differ.  It
compares two builds with each other and looks for nothing in particular.  CPU only: complements
``bench/refactor_equiv.py``, which compares what the two builds compute.

    python bench/kernel_isa.py dump parent.json [--keep-asm DIR]     # in the parent's checkout
    python bench/kernel_isa.py dump branch.json [--keep-asm DIR]     # in the branch's checkout
    python bench/kernel_isa.py compare parent.json branch.json --out report.json
"""
import argparse
import concurrent.futures as cf
import hashlib
import importlib.util
import json
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

META = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def _build_module():
    # madnn/ops/build.py of the checkout the command is run in, loaded by path: importing the package pulls in torch
    spec = importlib.util.spec_from_file_location("_madnn_build", Path.cwd() / "madnn" / "ops" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _normalise(body):
    labels, out = {}, []
    for line in body:
        line = re.sub(r"\s+", " ", line.split(";")[0].split("//")[0]).strip()
        if not line or (line.startswith(".") and not line.endswith(":")):
            continue
        line = re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), line)
        out.append(re.sub(r"\b_Z\w+", "SYM", line))
    return out


def _kernels(asm):
    """{mangled name: record} for every kernel of one assembly file."""
    lines = asm.splitlines()
    meta, cur = {}, None
    for line in lines[lines.index("amdhsa.kernels:"):]:
        m = re.match(r"^(  - |    )\.(\w+):\s+(\S+)$", line)
        if m and m.group(1) == "  - ":
            cur = {}
        if m and m.group(2) == "name":
            meta[m.group(3)] = cur
        elif m and m.group(2) in META:
            cur[m.group(2)] = int(m.group(3))
    out = {}
    for name, counts in meta.items():
        beg = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i in range(beg, len(lines)) if lines[i].startswith(".Lfunc_end"))
        stream = _normalise(lines[beg + 1:end])
        out[name] = {**counts, "instructions": sum(not l.endswith(":") for l in stream),
                     "hash": hashlib.sha256("\n".join(stream).encode()).hexdigest()[:16], "_stream": stream}
    return out


def _plain(mangled):
    name = subprocess.run(["c++filt", mangled], capture_output=True, text=True, check=True).stdout.strip()
    return re.sub(r"(\(anonymous namespace\)|\w+)::", "", name)


def dump(path, keep_asm):
    b = _build_module()

    def one(src):
        with tempfile.TemporaryDirectory() as tmp:
            s = Path(tmp) / (src + ".s")
            cmd = [b._hipcc(), *b._flags_kernels(), *b.EXTRA_FLAGS.get(src, []), "--offload-device-only", "-S",
                   str(b.CSRC / src), "-o", str(s)]
            res = subprocess.run(cmd, capture_output=True, text=True)
            if res.returncode != 0:
                raise RuntimeError(f"compile failed: {src}\n{res.stderr}")
            return src, _kernels(s.read_text())

    out = {}
    with cf.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 4)) as ex:
        for src, kernels in ex.map(one, [s for s in b.KERNEL_SOURCES if s.endswith(".hip")]):
            for mangled, rec in sorted(kernels.items()):
                key = f"{src}: {_plain(mangled)}"
                assert key not in out, f"two kernels named {key}"
                if keep_asm:
                    Path(keep_asm).mkdir(parents=True, exist_ok=True)
                    (Path(keep_asm) / (re.sub(r"\W+", "_", key) + ".s")).write_text("\n".join(rec["_stream"]) + "\n")
                out[key] = {k: v for k, v in rec.items() if k != "_stream"}
    Path(path).write_text(json.dumps(out, indent=1, sort_keys=True))
    print(f"{len(out)} kernels -> {path}")
    return 0


def compare(parent, branch, report):
    pa, br = json.loads(Path(parent).read_text()), json.loads(Path(branch).read_text())
    one_side = sorted(set(pa) ^ set(br))
    same = sorted(k for k in set(pa) & set(br) if pa[k] == br[k])
    differ = {k: {"parent": pa[k], "branch": br[k], "instruction_delta": br[k]["instructions"] - pa[k]["instructions"]}
              for k in sorted(set(pa) & set(br)) if pa[k] != br[k]}
    for k in one_side:
        print(f"ERROR: only in the {'parent' if k in pa else 'branch'}: {k}")
    for k in same:
        print(f"identical: {k}")
    for k, d in differ.items():
        print(f"DIFFERS: {k} ({d['instruction_delta']:+d} instructions)")
        print(f"  parent {d['parent']}\n  branch {d['branch']}")
    print(f"{len(same)} identical, {len(differ)} differ, {len(one_side)} on one side only")
    if report:
        Path(report).write_text(json.dumps({"kernels": len(set(pa) | set(br)), "identical": same, "differ": differ,
                                            "one_side_only": one_side}, indent=1))
    return 1 if one_side or differ else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    dp = sub.add_parser("dump")
    dp.add_argument("path")
    dp.add_argument("--keep-asm", metavar="DIR", help="also write every kernel's normalised stream here")
    cp = sub.add_parser("compare")
    cp.add_argument("parent")
    cp.add_argument("branch")
    cp.add_argument("--out")
    args = ap.parse_args()
    sys.exit(dump(args.path, args.keep_asm) if args.cmd == "dump" else compare(args.parent, args.branch, args.out))
