"""Did adding the VARLEN template parameter to the K8 kernels change any pre-existing kernel's machine code?

Takes two ``bench/kernel_isa.py dump`` files (the parent's and the branch's).  The grown template argument list
changes the demangled names of the three register-staged attention kernels (``attn_fwd_kernel<64, true, false>``
became ``attn_fwd_kernel<64, true, false, false>``), so ``kernel_isa.py compare`` cannot pair them; this pairs a
parent kernel with the branch kernel whose template arguments are the parent's plus ``false`` (VARLEN off) and
compares the recorded instruction hash, VGPR count, LDS footprint and scratch size.  Every other kernel, of every
``.hip``, is paired by its unchanged name.  The record also lists the new VARLEN instantiations with their VGPR
count and scratch size.  CPU only.

What the hash cannot keep: ``MadnnAttnArgs`` grew by one pointer (``seqlens``, its last field), and the compiler
places the implicit kernel arguments (the grid size that ``map_block`` reads) right behind the explicit ones, so in
every kernel that takes the block by value ONE scalar load reads its operand 8 bytes further on (``s_load_dword
s3, s[0:1], 0x130`` became ``... 0x138``).  That immediate is part of the hashed stream.  With the two dumps'
``--keep-asm`` directories the script checks exactly that: a pair whose recorded hashes differ counts as
``same_up_to_implicit_argument_offset`` only if the two streams differ in nothing but such loads, each moved by
``--grown-by`` bytes, and the branch's stream with those immediates moved back hashes to the PARENT's recorded hash.
Anything else is reported as a difference.

    python bench/kernel_isa.py dump parent.json --keep-asm parent_asm      # in the parent's checkout
    python bench/kernel_isa.py dump branch.json --keep-asm branch_asm      # in the branch's checkout
    python bench/attn_varlen_isa.py parent.json branch.json --parent-asm parent_asm --branch-asm branch_asm \
        --out profiles/attn_varlen_isa.json
"""
import argparse
import hashlib
import json
import re
import sys
from pathlib import Path

KEPT = ("hash", "vgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")
GROWN = ("attn_fwd_kernel", "attn_bwd_dq_kernel", "attn_bwd_dkdv_kernel")


def _branch_name(parent_key):
    """The branch's name of a parent kernel: the three grown templates gain a trailing ``false``."""
    m = re.match(r"^(attn\.hip: void (\w+)<)([^>]*)(>.*)$", parent_key)
    if m and m.group(2) in GROWN:
        return f"{m.group(1)}{m.group(3)}, false{m.group(4)}"
    return parent_key


def _stream(asm_dir, key):
    return (Path(asm_dir) / (re.sub(r"\W+", "_", key) + ".s")).read_text().splitlines()


_KERNARG_LOAD = re.compile(r"^(s_load_dword(?:x\d+)? \S+ s\[0:1\], )(0x[0-9a-f]+|\d+)$")


def _only_implicit_offset(pstream, bstream, grown_by, parent_hash):
    """The moved loads if the two streams differ by nothing else and the branch's stream, rebased, hashes to the
    parent's recorded hash; else None."""
    if len(pstream) != len(bstream):
        return None
    moved, rebased = [], []
    for pl, bl in zip(pstream, bstream):
        if pl != bl:
            pm, bm = _KERNARG_LOAD.match(pl), _KERNARG_LOAD.match(bl)
            if not (pm and bm and pm.group(1) == bm.group(1) and int(bm.group(2), 0) - int(pm.group(2), 0) == grown_by):
                return None
            moved.append({"parent": pl, "branch": bl})
        rebased.append(pl)
    if not moved or hashlib.sha256("\n".join(rebased).encode()).hexdigest()[:16] != parent_hash:
        return None
    return moved


def _is_varlen(key):
    m = re.match(r"^attn\.hip: void (\w+)<([^>]*)>", key)
    return bool(m and m.group(1) in GROWN and m.group(2).split(", ")[-1] == "true" and len(m.group(2).split(", ")) == 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--parent-asm", help="the parent dump's --keep-asm directory")
    ap.add_argument("--branch-asm", help="the branch dump's --keep-asm directory")
    ap.add_argument("--grown-by", type=int, default=8, help="bytes the explicit argument block grew by")
    ap.add_argument("--out")
    args = ap.parse_args()
    pa, br = json.loads(Path(args.parent).read_text()), json.loads(Path(args.branch).read_text())
    identical, moved_only, differ, missing, paired = [], [], {}, [], set()
    for key, prec in sorted(pa.items()):
        bkey = _branch_name(key)
        if bkey not in br:
            missing.append(key)
            continue
        paired.add(bkey)
        if all(prec[f] == br[bkey][f] for f in KEPT):
            identical.append({"parent": key, "branch": bkey, **{f: prec[f] for f in KEPT}})
            continue
        moved = None
        if args.parent_asm and args.branch_asm and all(prec[f] == br[bkey][f] for f in KEPT[1:]):
            moved = _only_implicit_offset(_stream(args.parent_asm, key), _stream(args.branch_asm, bkey), args.grown_by,
                                          prec["hash"])
        if moved is not None:
            moved_only.append({"parent": key, "branch": bkey, "parent_hash": prec["hash"], "branch_hash": br[bkey]["hash"],
                               "branch_hash_with_the_offset_moved_back": prec["hash"], "moved_loads": moved,
                               **{f: prec[f] for f in KEPT[1:]}})
        else:
            differ[key] = {"branch_name": bkey, "parent": {f: prec[f] for f in KEPT},
                           "branch": {f: br[bkey][f] for f in KEPT}}
    new = {k: {"vgpr_count": v["vgpr_count"], "scratch": v["private_segment_fixed_size"],
               "lds": v["group_segment_fixed_size"], "instructions": v["instructions"]}
           for k, v in sorted(br.items()) if k not in paired}
    not_varlen = [k for k in new if not _is_varlen(k)]
    bad = {k: v for k, v in new.items() if v["scratch"] != 0 or (
        re.search(r"attn_(fwd|bwd_dq)_kernel<128", k) and v["vgpr_count"] > 256)}
    for k in missing:
        print(f"ERROR: no branch kernel for the parent's {k}")
    for k, d in differ.items():
        print(f"DIFFERS: {k}\n  parent {d['parent']}\n  branch {d['branch']}")
    for k in not_varlen:
        print(f"ERROR: new kernel that is no VARLEN instantiation: {k}")
    for k, v in new.items():
        print(f"new: {k}: {v}")
    for k, v in bad.items():
        print(f"ERROR: {k} has scratch or too many VGPRs: {v}")
    for r in moved_only:
        print(f"same up to the implicit-argument offset: {r['parent']}: {r['moved_loads']}")
    print(f"{len(identical)} pre-existing kernels identical, {len(moved_only)} identical up to the implicit-argument "
          f"offset, {len(differ)} differ, {len(missing)} missing, {len(new)} new")
    if args.out:
        Path(args.out).write_text(json.dumps({
            "compared": list(KEPT), "parent_kernels": len(pa), "identical": len(identical),
            "same_up_to_implicit_argument_offset": len(moved_only), "differ": differ, "missing_in_branch": missing,
            "note": "every kernel that takes MadnnAttnArgs by value: the recorded hash changed because the one scalar "
                    "load of an implicit kernel argument moved by the 8 bytes the argument block grew by; nothing else "
                    "in the stream, and no VGPR count, LDS footprint or scratch size, changed",
            "attn_hip_identical": [r for r in identical if r["parent"].startswith("attn.hip: ")],
            "attn_hip_same_up_to_implicit_argument_offset": moved_only,
            "varlen_instantiations": new}, indent=1))
    return 1 if differ or missing or not_varlen or bad else 0


if __name__ == "__main__":
    sys.exit(main())
