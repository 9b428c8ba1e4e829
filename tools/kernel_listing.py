"""Resource usage of every gfx950 kernel of one or more device-assembly files, as CSV on stdout (sorted by name): the fields of
the amdhsa.kernels metadata plus the instruction count of the kernel body.  Two source layouts that must compile to the same
kernels (a refactor) give identical listings:
    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S vq_seg_amd/csrc/conv_patch.hip -o patch.s
    python tools/kernel_listing.py patch.s [more.s ...] > listing.csv"""
import re, sys
FIELDS = ["vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"]
rows = {}
for path in sys.argv[1:]:
    text = open(path).read()
    # instructions between a function's label and its .Lfunc_end label (directives and comments not counted)
    insts = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, flags=re.S | re.M):
        body = m.group(2)
        n = sum(1 for l in body.split("\n") if re.match(r"^\t[a-z]\w*(\s|$)", l) and not l.startswith("\t."))
        insts[m.group(1)] = n
    meta = text[text.index("amdhsa.kernels:"):]
    for blk in re.split(r"^  - ", meta, flags=re.M)[1:]:
        blk = "    " + blk
        m = re.search(r"^    \.name:\s+(\S+)", blk, flags=re.M)
        if not m: continue                                   # (amdhsa.version's list items)
        name = m.group(1)
        vals = [re.search(r"^    \.%s:\s+(\d+)" % f, blk, flags=re.M) for f in FIELDS]
        rows[name] = [v.group(1) if v else "" for v in vals] + [str(insts.get(name, -1))]
print("kernel," + ",".join(FIELDS) + ",instructions")
for name in sorted(rows):
    print(name + "," + ",".join(rows[name]))
