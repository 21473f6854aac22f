#!/usr/bin/env python3
"""Developer probe (CPU only): instruction classes per kernel of one .hip unit, whole kernel and per basic block.
    tools/isa_count.py x266_amd/csrc/dct32_kernels.hip [name-substring] [--blocks]
Compiles the device side to assembly with the product's flags and counts VALU / MFMA / DS / VMEM / SALU / s_waitcnt; the
register counts, the scratch size and the static LDS size are each kernel's own entry of the amdhsa.kernels metadata.
With --blocks every basic block (label to label) of the matching kernels is listed, so a steady-state loop can be read off.
A .s file (the same flags' output, kept from another revision) is counted as it is."""
import collections, os, re, subprocess, sys, tempfile

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-amdgpu-mfma-vgpr-form", "-S", "--cuda-device-only"]
META = (("vgprs", "vgpr_count"), ("sgprs", "sgpr_count"), ("scratch", "private_segment_fixed_size"), ("lds", "group_segment_fixed_size"))


def classify(op):
    if op.startswith("v_mfma"): return "mfma"
    if op.startswith("v_"): return "valu"
    if op.startswith("ds_"): return "ds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")): return "vmem"
    if op.startswith("s_waitcnt"): return "waitcnt"
    if op.startswith("s_load") or op.startswith("s_buffer_load"): return "smem"
    if op.startswith("s_"): return "salu"
    return None


def assembly(src):
    if src.endswith(".s"): return open(src).read()
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + ["-o", out, src], check=True, stderr=subprocess.DEVNULL)
        return open(out).read()


def metadata(txt):
    """{kernel name: {"vgprs": .., "sgprs": .., "scratch": .., "lds": ..}} from the amdhsa.kernels list (one `  - ` entry per kernel)"""
    meta = {}
    for entry in txt.partition("amdhsa.kernels:")[2].split("\n  - ")[1:]:
        name = re.search(r"\n    \.name:\s*(\S+)", entry)
        if not name: continue
        meta[name.group(1)] = {k: int(re.search(r"\n    \.%s:\s*(\d+)" % f, entry).group(1)) for k, f in META}
    return meta


def kernels(txt):
    """[(name, total counts, [(block label, counts)], metadata entry)] in file order"""
    meta = metadata(txt)
    parts = re.split(r"\n(_Z[^\n:]*):[^\n]*\n", txt)
    res = []
    for i in range(1, len(parts), 2):
        name, body = parts[i], parts[i + 1].split(".Lfunc_end")[0]
        total = collections.Counter()
        cur_label, cur = "entry", collections.Counter()
        per_block = []
        for line in body.split("\n"):
            line = line.strip()
            m = re.match(r"(\.LBB[0-9_]+):", line)
            if m:
                per_block.append((cur_label, cur)); cur_label, cur = m.group(1), collections.Counter()
                continue
            m = re.match(r"([a-z_0-9]+)", line)
            if not m or line.startswith((".", ";")): continue
            k = classify(m.group(1))
            if k: total[k] += 1; cur[k] += 1
        per_block.append((cur_label, cur))
        res.append((name, total, per_block, meta.get(name, {})))
    return res


def main():
    want = [a for a in sys.argv[2:] if not a.startswith("--")]
    blocks = "--blocks" in sys.argv
    for name, total, per_block, meta in kernels(assembly(sys.argv[1])):
        if want and not any(w in name for w in want): continue
        print("%s\n   total %s  %s" % (name, dict(total), "  ".join("%s %s" % (k, meta.get(k, "?")) for k, _ in META)))
        if blocks:
            for lab, c in per_block:
                if sum(c.values()) > 8: print("   %-12s %s" % (lab, dict(c)))


if __name__ == "__main__":
    main()
