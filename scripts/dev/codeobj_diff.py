#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds, kernel by kernel:
    scripts/dev/codeobj_diff.py PARENT_CSRC RESULT_CSRC [--focus REGEX] [--json OUT]
Both arguments are directories of compiled objects (*.o, as `make -C libwave_amd/csrc` leaves them).
Per kernel: the resources from the code object's notes (what scripts/dev/kres.sh prints), an occupancy
derived from them (waves per SIMD: 512 registers in granules of 8, at most 8; workgroups per CU by LDS:
160 KiB), and the disassembly (llvm-objdump -d) with addresses and branch targets stripped.  Kernels
matching --focus are always listed; the others only when something differs.  --json writes the report as it
stands under "device_code" in profiles/nn_split_vs_parent.json (the other keys of that file are measurements
added beside it)."""
import collections, glob, json, os, re, subprocess, sys, tempfile

LLVM = "/opt/rocm/lib/llvm/bin/"
KEYS = ["vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
        "private_segment_fixed_size", "group_segment_fixed_size"]


def code_object(obj, tmp):
    fat = os.path.join(tmp, "fat.bin")
    co = os.path.join(tmp, os.path.basename(obj) + ".co")
    if subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat]).returncode or not os.path.getsize(fat):
        return None
    lst = subprocess.run([LLVM + "clang-offload-bundler", "--list", "--type=o", "--input=" + fat],
                         capture_output=True, text=True).stdout.split()
    tgt = [t for t in lst if "gfx950" in t]
    if not tgt:
        return None
    subprocess.check_call([LLVM + "clang-offload-bundler", "--type=o", "--targets=" + tgt[0], "--input=" + fat,
                           "--output=" + co, "--unbundle"])
    return co


def kernels_of(csrc):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sorted(glob.glob(os.path.join(csrc, "*.o"))):
            co = code_object(obj, tmp)
            if not co:
                continue
            notes = subprocess.run([LLVM + "llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
            res = {}
            for blk in notes.split("  - .agpr_count:")[1:]:
                blk = ".agpr_count:" + blk
                g = lambda k: (re.search(r"\.%s:\s+(\S+)" % k, blk) or [None, "?"])[1]
                name = re.search(r"\.name:\s+(\S+)", blk).group(1)
                res[name] = {k: g(k) for k in KEYS}
            dis = subprocess.run([LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True).stdout
            cur = None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if m:
                    cur = m.group(1) if m.group(1) in res else None
                    if cur:
                        res[cur]["_insn"] = []
                    continue
                if cur and line[:1] in " \t" and line.strip():
                    t = line.split("//")[0].strip()
                    t = re.sub(r"\s+", " ", t)
                    if t == "...":
                        continue  # (objdump's mark for a run of zero words, in the padding between kernels)
                    if re.match(r"^(s_cbranch|s_branch|s_call)", t):
                        t = t.split(" ")[0]
                    res[cur]["_insn"].append(t)
            for name, r in res.items():
                # (padding behind a kernel's last instruction: s_code_end, and the s_nop that align the next kernel;
                # an s_nop inside the code is a hazard wait and stays)
                while r.get("_insn") and re.match(r"^(s_nop|s_code_end)", r["_insn"][-1]):
                    r["_insn"].pop()
                r.setdefault("_insn", [])
                r["_obj"] = os.path.basename(obj)
                out[name] = r
    return out


def demangle(name):
    try:
        return subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    except OSError:
        return name


def occupancy(r):
    try:
        regs = int(r["vgpr_count"]) + int(r["agpr_count"])
        lds = int(r["group_segment_fixed_size"])
    except ValueError:
        return "?"
    waves = min(8, 512 // max(8, (regs + 7) // 8 * 8))
    return {"waves_per_simd_by_registers": waves, "workgroups_per_cu_by_lds": (163840 // lds) if lds else None}


def main():
    args = [a for a in sys.argv[1:]]
    focus, jout = None, None
    if "--focus" in args:
        i = args.index("--focus"); focus = re.compile(args[i + 1]); del args[i:i + 2]
    if "--json" in args:
        i = args.index("--json"); jout = args[i + 1]; del args[i:i + 2]
    A, B = kernels_of(args[0]), kernels_of(args[1])
    rep = {"kernels": len(B), "only_in_parent": sorted(set(A) - set(B)), "only_in_result": sorted(set(B) - set(A)),
           "moved_between_objects": [], "listed": {}, "others_identical": True}
    for name in sorted(set(A) & set(B)):
        a, b = A[name], B[name]
        same_seq = a["_insn"] == b["_insn"]
        same_res = all(a[k] == b[k] for k in KEYS if k != "sgpr_count")  # (scalar registers: recorded, not a condition)
        moved = a["_obj"] != b["_obj"]
        if moved:
            rep["moved_between_objects"].append(name)
        if (focus and focus.search(name)) or not (same_seq and same_res):
            if not (focus and focus.search(name)):
                rep["others_identical"] = False
            rep["listed"][name] = {
                "object": [a["_obj"], b["_obj"]],
                "parent": dict({k: a[k] for k in KEYS}, occupancy=occupancy(a)),
                "result": dict({k: b[k] for k in KEYS}, occupancy=occupancy(b)),
                "same_resources": same_res and occupancy(a) == occupancy(b),
                "none_above_parent": all(int(b[k]) <= int(a[k]) for k in KEYS if k != "sgpr_count" and a[k] != "?" and b[k] != "?"),
                "instructions": [len(a["_insn"]), len(b["_insn"])],
                "same_instruction_sequence": same_seq,
                "same_instruction_multiset": collections.Counter(a["_insn"]) == collections.Counter(b["_insn"]),
            }
    for name, e in rep["listed"].items():
        a, b = A[name], B[name]
        print("%s res %s seq %s multiset %s  %d -> %d  v%s/%s lds %s  %s" % (
            "same " if e["same_resources"] else ("lower" if e["none_above_parent"] else "ABOVE"), e["same_resources"], e["same_instruction_sequence"],
            e["same_instruction_multiset"], e["instructions"][0], e["instructions"][1], e["parent"]["vgpr_count"],
            e["result"]["vgpr_count"], e["result"]["group_segment_fixed_size"],
            demangle(name)[:90]), [(k, a[k], b[k]) for k in KEYS if a[k] != b[k]])
    print("kernels %d, only in parent %s, only in result %s, others identical: %s" % (
        rep["kernels"], rep["only_in_parent"], rep["only_in_result"], rep["others_identical"]))
    if jout:
        json.dump(rep, open(jout, "w"), indent=1)


if __name__ == "__main__":
    main()
