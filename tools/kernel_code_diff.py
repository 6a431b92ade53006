"""Are the kernels of two hipcc objects / shared libraries the same machine code?  For a refactor that renames kernel instantiations.

Every gfx950 code object of A and of B is disassembled (rba_amd/csrc/isa_hazards.py::disassemble), the listing is cut at the symbol labels, symbol names are
dropped, and the instruction bodies are compared AS A MULTISET: same number of kernels / functions, no body on one side only.  The same for the kernel descriptors
(llvm-readelf --notes: register counts, LDS and scratch bytes, workgroup size), keyed by body.  Exit status 1 on any difference.

Usage: python tools/kernel_code_diff.py A B [A2 B2 ...]"""
import collections
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rba_amd", "csrc"))
import isa_hazards  # noqa: E402

FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".max_flat_workgroup_size")


def descriptors(path):
    """{kernel symbol: (the FIELDS of its descriptor)} over every gfx950 code object of `path`"""
    tmp, out = tempfile.mkdtemp(prefix="kcd_"), {}
    try:
        shutil.copy(path, os.path.join(tmp, "x.bin"))
        subprocess.run([os.path.join(isa_hazards.LLVM, "llvm-objdump"), "--offloading", "x.bin"], cwd=tmp, check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL)
        for f in sorted(os.listdir(tmp)):
            if "amdgcn" not in f:
                continue
            txt = subprocess.run([os.path.join(isa_hazards.LLVM, "llvm-readelf"), "--notes", os.path.join(tmp, f)], check=True, stdout=subprocess.PIPE,
                                 text=True).stdout
            for entry in re.split(r"\n  - ", txt):                         # one list item of amdhsa.kernels per kernel; its own keys are indented by four
                kv = dict(re.findall(r"^(?:    )?\.([a-z_]+):\s+(\S+)\s*$", entry, re.M))
                if "name" in kv and "vgpr_count" in kv:
                    out[kv["name"].strip("'\"")] = tuple(kv.get(k[1:]) for k in FIELDS)
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def bodies(path):
    """Counter of (body hash, descriptor) over every symbol of every code object, and one (name, length) per entry for the report"""
    desc, count, names = descriptors(path), collections.Counter(), {}
    for _, ins in isa_hazards.disassemble(path):
        cur, name = None, None

        def flush():
            if cur is not None:
                key = (hashlib.sha1("\n".join(cur).encode()).hexdigest()[:16], desc.get(name))
                count[key] += 1
                names.setdefault(key, (name, len(cur)))

        for text, kernel in ins:
            if text == "label":
                flush()
                cur, name = [], kernel
            else:
                cur.append(re.sub(r"<[^>]*>", "", text))                  # branch targets are printed as <symbol+offset>
        flush()
    return count, names


def main(argv):
    if len(argv) < 2 or len(argv) % 2:
        print(__doc__)
        return 2
    bad = 0
    for pa, pb in zip(argv[0::2], argv[1::2]):
        a, an = bodies(pa)
        b, bn = bodies(pb)
        only_a, only_b = a - b, b - a
        nk = sum(1 for k in a.elements() if k[1] is not None)
        print(f"{os.path.basename(pa)}: {sum(a.values())} / {sum(b.values())} bodies ({nk} kernels with descriptors), {len(a)} / {len(b)} distinct; "
              f"only in A: {sum(only_a.values())}, only in B: {sum(only_b.values())}")
        for side, only, nm in (("A", only_a, an), ("B", only_b, bn)):
            for k in list(only)[:10]:
                print(f"  {side} {nm[k][0][:140]} ({nm[k][1]} instructions) {k[1]}")
        bad += bool(only_a or only_b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
