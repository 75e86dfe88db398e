r"""Per-kernel gfx950 ISA of one HIP source, for "this change leaves the existing kernels' code unchanged"
checks (round 6: the 16-bit format templates of llama_kernels.hip / attn_kernels.hip).

    python scripts/diag/isa_compare.py dump <src.hip> <out.json>      # kernel -> normalised instructions
    python scripts/diag/isa_compare.py diff <before.json> <after.json> [--map OLD=NEW ...]

``--re PATTERN=REPL`` applies a regular-expression substitution instead, e.g. for the ``_docs`` kernels
folded into the plain templates as a fourth parameter ``DOC``:

    --re '_docs_kernel<(\d), (true|false)>=_kernel<false, \1, \2, true>'
    --re '(attn_(?:fwd|dq|dkdv)_kernel<(?:true|false), \d, (?:true|false))>=\1, false>'

``dump`` compiles the source to device assembly with the library's flags and keeps, per kernel
symbol, its instruction lines with basic-block labels and comments stripped (labels are renumbered
between builds). ``diff`` pairs kernels by demangled name after applying ``--map`` substitutions
(a template parameter added with its old value, e.g. ``--map "<4, false>=<4, false, 0>"``) and prints
identical / differing / unmatched kernels; for a differing kernel also the per-mnemonic count deltas and
its register, scratch and LDS figures (the assembly metadata's, kept by ``dump``) before and after, and
where it differs: the first and last differing instruction and how many of the diff blocks lie between
the first and last ``v_mfma`` (the hot loop). Exit status 1 when any paired kernel differs."""
import difflib
import json
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


META = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def dump(src, out):
    from sparse_matrix_tuning_amd import build
    flags = build.FILE_FLAGS.get(os.path.basename(src), [])
    with tempfile.TemporaryDirectory() as d:
        s = os.path.join(d, "k.s")
        cmd = [build.hipcc(), f"--offload-arch={build.ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function",
               "-I", os.path.join(ROOT, "include"), *flags, "--cuda-device-only", "-S", "-o", s, src]
        subprocess.run(cmd, check=True)
        text = open(s).read()
    kernels, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^([_A-Za-z][\w.$]*):\s*(;.*)?$", line)
        if m and not m.group(1).startswith((".L", "$")):
            cur = m.group(1)
            kernels[cur] = []
            continue
        if cur is None:
            continue
        if line.startswith(("\t.end_amdhsa_kernel", ".Lfunc_end", "\t.section", "\t.amdgpu_metadata")):
            cur = None
            continue
        ins = line.split(";")[0].strip()
        if not ins or ins.startswith(".") or re.match(r"^\.?L\w+:", ins):
            continue
        kernels[cur].append(re.sub(r"\.LBB\d+_\d+", ".LBB", ins))
    # the metadata's per-kernel resource figures: 4-space "key: value" lines of the block that holds .name
    meta, block = {}, {}
    for line in text[text.find("amdhsa.kernels:"):].splitlines()[1:]:
        if line.startswith("  - ") or not line.startswith(" "):
            meta[block.get(".name")] = {k: int(block[k]) for k in META if k in block}
            block = {}
            if not line.startswith(" "):
                break
        m = re.match(r"^(?:  - |    )(\.\w+):\s*(\S+)\s*$", line)
        if m:
            block[m.group(1)] = m.group(2)
    names = subprocess.run(["c++filt"], input="\n".join(kernels), capture_output=True, text=True).stdout.split("\n")
    res = {dm: {"ins": kernels[k], "meta": meta.get(k, {})} for k, dm in zip(kernels, names) if kernels[k] and "(" in dm}
    json.dump(res, open(out, "w"))
    print(f"{len(res)} kernels -> {out}")


def diff(a, b, maps):
    # a dump from before the metadata was kept is a bare instruction list per kernel
    A, B = ({n: v if isinstance(v, dict) else {"ins": v, "meta": {}} for n, v in json.load(open(f)).items()} for f in (a, b))
    sub = [(m[0], m[1].split("=", 1)) for m in maps]

    def key(n):
        for kind, (old, new) in sub:
            n = re.sub(old, new, n) if kind == "re" else n.replace(old, new)
        return n
    Am = {key(n): v for n, v in A.items()}
    same, differ, missing = [], [], []
    for n, v in Am.items():
        if n not in B:
            missing.append(n)
        elif B[n]["ins"] == v["ins"]:
            same.append(n)
        else:
            differ.append(n)
    for n in same:
        print("identical ", n)
    for n in differ:
        print("DIFFERENT ", n, len(Am[n]["ins"]), len(B[n]["ins"]))
        ca, cb = (Counter(i.split()[0] for i in k[n]["ins"]) for k in (Am, B))
        print("    counts:", " ".join(f"{m} {cb[m] - ca[m]:+d}" for m in sorted(ca | cb) if ca[m] != cb[m]) or "equal")
        print("    meta:  ", " ".join(f"{k} {Am[n]['meta'].get(k)} -> {B[n]['meta'].get(k)}" for k in META))
        # where it differs (indices into the listing before): did the hot loop move?
        ia = Am[n]["ins"]
        blocks = [op for op in difflib.SequenceMatcher(None, ia, B[n]["ins"], autojunk=False).get_opcodes()
                  if op[0] != "equal"]
        mf = [i for i, x in enumerate(ia) if x.startswith("v_mfma")]
        hot = sum(1 for _, i1, i2, _, _ in blocks if mf and i1 <= mf[-1] and max(i2, i1 + 1) > mf[0])
        print(f"    where:   first {blocks[0][1]}, last {max(blocks[-1][2] - 1, blocks[-1][1])} of {len(ia)}; "
              f"{len(blocks)} diff blocks, {hot} between the first and last v_mfma"
              + (f" ({mf[0]}..{mf[-1]})" if mf else ""))
    for n in missing:
        print("unmatched ", n)
    print(f"{len(same)} identical, {len(differ)} different, {len(missing)} unmatched of {len(Am)} before; "
          f"{len(B)} kernels after")
    return 1 if differ else 0


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2], sys.argv[3])
    else:
        maps = [(x[2:], sys.argv[i + 1]) for i, x in enumerate(sys.argv) if x in ("--map", "--re")]
        sys.exit(diff(sys.argv[2], sys.argv[3], maps))
