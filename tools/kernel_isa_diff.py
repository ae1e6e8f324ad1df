"""Machine code of every gfx950 kernel of two builds of the same objects, side by side (no GPU needed):
   python tools/kernel_isa_diff.py <parent build dir> <tree build dir> kernels_match.o kernels_match_16bit.o ... [old_name=new_name ...]
For each kernel of each object: class A (the same instruction list and the same resource line), B (the same mnemonic histogram and
resource line, another order or other register numbers) or C (anything else); then the instruction counts and the resource lines
(vgpr/agpr/sgpr/vspill/sspill/lds/scratch, as tools/kernel_resources.py prints them) of both builds.  `old=new` pairs follow a kernel
that was renamed: `old` and `new` are prefixes of the demangled name up to the template arguments they replace, e.g.
'l2_knn2_half_kernel<16, 12, 2, 4, 2, =l2_knn2_levels_kernel<16, 12, 2, 4, 2, 3, '.  Exit status 1 if a kernel is in class C or
exists in one build only."""
import collections, os, re, subprocess, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from regard3d_amd import codeobj

LLVM = "/opt/rocm/lib/llvm/bin/"


def kernels_of(path):
    """{demangled kernel name: (instruction lines, resource line)}"""
    out = {}
    for co in codeobj._code_objects(open(path, "rb").read()):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co); f.flush()
            notes = subprocess.run([LLVM + "llvm-readelf", "--notes", f.name], capture_output=True, text=True).stdout
            dis = subprocess.run([LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", f.name], capture_output=True, text=True).stdout
        res = {}
        for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
            blk = ".agpr_count:" + blk
            g = lambda k: (re.search(r"\." + k + r":\s*(\S+)", blk) or [None, "?"])[1]
            res[g("name")] = "/".join(g(k) for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                                                     "group_segment_fixed_size", "private_segment_fixed_size"))
        for m in re.finditer(r"^[0-9a-f]+ <([^>]+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, re.S | re.M):
            if m.group(1) not in res:
                continue
            ins = [re.sub(r"\s*//.*", "", l).strip() for l in m.group(2).splitlines()]
            ins = [l for l in ins if l and not l.endswith(":") and not l.startswith(";")]
            while ins and ins[-1] in ("s_nop 0", "..."):     # the padding up to the next kernel's alignment: not this kernel's code
                ins.pop()
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            out[re.sub(r"\(.*", "", name).replace("void r3dm::", "").replace("r3dm::", "")] = (ins, res[m.group(1)])
    return out


def main():
    parent, tree = sys.argv[1], sys.argv[2]
    objs = [a for a in sys.argv[3:] if "=" not in a]
    renames = [a.split("=", 1) for a in sys.argv[3:] if "=" in a]
    bad = 0
    print("class  instructions parent -> tree   vgpr/agpr/sgpr/vspill/sspill/lds/scratch parent -> tree   kernel (tree's name)")
    for o in objs:
        kp, kt = kernels_of(os.path.join(parent, o)), kernels_of(os.path.join(tree, o))
        for old, new in renames:
            for k in [k for k in kp if k.startswith(old)]:
                kp[new + k[len(old):]] = kp.pop(k)
        print(f"## {o}: {len(kp)} kernels in the parent, {len(kt)} in the tree")
        for k in sorted(set(kp) | set(kt)):
            if k not in kp or k not in kt:
                print(f"  -    only in the {'tree' if k in kt else 'parent'}: {k}"); bad = 1
                continue
            (ip, rp), (it, rt) = kp[k], kt[k]
            hist = lambda ins: collections.Counter(l.split()[0] for l in ins)
            cls = "A" if ip == it and rp == rt else "B" if hist(ip) == hist(it) and rp == rt else "C"
            bad |= cls == "C"
            print(f"  {cls}    {len(ip):6d} -> {len(it):6d}   {rp} -> {rt}   {k}")
    sys.exit(bad)


if __name__ == "__main__":
    main()
