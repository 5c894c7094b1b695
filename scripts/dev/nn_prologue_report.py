#!/usr/bin/env python3
"""What a wave of the search kernels does before its walk starts, read from the gfx950 code object:
    scripts/dev/nn_prologue_report.py [CSRC_DIR] [--md]
Cross-compiles CSRC_DIR/wm_nn.hip and wm_nn_cert.hip (default: libwave_amd/csrc of this tree) to assembly with the
Makefile's flags (--cuda-device-only -S; no GPU needed) and prints, for every instantiation of k_nn_grid and k_nn_cert:
  waits<VL   s_waitcnt instructions that wait for scalar loads (lgkmcnt) in front of the first vector load, in program
             order: the dependent scalar round trips a wave makes before it requests its first stream
  br<VL      conditional branches in front of the first vector load (a `done` test there is one)
  streams    the prologue's stream loads: the first 3 vector loads of k_nn_grid (source point, key, match), the
             first 3 NB of k_nn_cert (source point, match, bound, NB batches), as "first..last" line distance
  vm-between whether a wait on vector loads (vmcnt) or a branch sits between the first and the last of them
  state<VL   scalar loads of the state (an s_load whose base is not the kernarg pointer s[0:1]) in front of the first
             vector load: a `done` word fetched and waited for before the streams are requested shows here
  VL..state  s_waitcnt instructions between the first stream load and the last scalar load of the state in the
             prologue (up to 40 instructions behind the last stream load): 0 = the state is requested together
             with the streams, before anything is waited for
  sqrt       v_sqrt_f32 in the kernel: raw / with the library's correction sequence behind it (the IEEE sqrtf: scale,
             v_sqrt_f32, two v_fma corrections, v_cmp_class)
  resources  vgprs, agprs, sgprs, spilled vgprs, scratch bytes per lane, LDS bytes, waves per SIMD by registers
The code object is the judge of the prologue, not the source: this is the check the source's comments point to."""
import os, re, subprocess, sys

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Wall -Wno-unused-result".split()  # the Makefile's
VLOAD = re.compile(r"^(global_load|buffer_load|flat_load|scratch_load)")


def assembly(path):
    r = subprocess.run([HIPCC] + FLAGS + ["--cuda-device-only", "-S", path, "-o", "-"], capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr)
    return r.stdout


def demangle(name):
    for tool in ("/opt/rocm/lib/llvm/bin/llvm-cxxfilt", "c++filt"):
        try:
            return subprocess.run([tool, name], capture_output=True, text=True).stdout.strip()
        except OSError:
            pass
    return name


def kernels(asm):
    """name -> list of instructions (comments and labels dropped), for k_nn_grid / k_nn_cert"""
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(_ZN2wm9k_nn_(?:grid|cert)\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        t = line.split(";")[0].strip()
        if not t or t.endswith(":") or t.startswith("."):
            continue
        out[cur].append(re.sub(r"\s+", " ", t))
    return out


def resources(asm):
    res = {}
    for blk in asm.split("  - .agpr_count:")[1:]:
        blk = ".agpr_count:" + blk
        g = lambda k: int((re.search(r"\.%s:\s+(\d+)" % k, blk) or [None, "-1"])[1])
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        res[name] = {k: g(k) for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count",
                                        "private_segment_fixed_size", "group_segment_fixed_size")}
    return res


def analyse(name, ins):
    dem = demangle(name)
    short = re.sub(r"\(.*", "", dem).replace("void wm::", "")
    if "k_nn_cert" in short:
        nb = int(re.search(r"k_nn_cert<[^,]+, (\d+)", short).group(1))
        n_streams = 3 * nb
    else:
        n_streams = 3
    vl = [k for k, t in enumerate(ins) if VLOAD.match(t) and not t.startswith("scratch_load")]
    first, last = vl[0], vl[n_streams - 1]
    before = ins[:first]
    waits = sum(1 for t in before if t.startswith("s_waitcnt") and "lgkmcnt" in t)
    branches = sum(1 for t in before if t.startswith("s_cbranch"))
    between = ins[first:last + 1]
    vm_between = any((t.startswith("s_waitcnt") and "vmcnt" in t) or t.startswith("s_cbranch") for t in between)
    state = [k for k, t in enumerate(ins[:last + 40]) if re.match(r"^s_load_\w+ \S+ s\[(?!0:1\])", t)]
    state_front = sum(1 for k in state if k < first)
    waits_to_state = sum(1 for t in ins[first:max(state)] if t.startswith("s_waitcnt")) if state and max(state) > first else 0
    raw = corrected = 0
    for k, t in enumerate(ins):
        if t.startswith("v_sqrt_f32"):
            if any(u.startswith("v_cmp_class_f32") for u in ins[k + 1:k + 20]):
                corrected += 1
            else:
                raw += 1
    return {"kernel": short, "waits_before_first_vload": waits, "branches_before_first_vload": branches,
            "streams": "%d..%d" % (first, last), "wait_or_branch_between_streams": vm_between,
            "state_loads_before_first_vload": state_front, "waits_first_stream_to_last_state_load": waits_to_state,
            "sqrt_raw": raw, "sqrt_corrected": corrected, "instructions": len(ins)}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    md = "--md" in sys.argv
    csrc = args[0] if args else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "libwave_amd", "csrc")
    rows = []
    for f in ("wm_nn.hip", "wm_nn_cert.hip"):
        asm = assembly(os.path.join(csrc, f))
        res = resources(asm)
        for name, ins in kernels(asm).items():
            r = analyse(name, ins)
            r.update(res.get(name, {}))
            regs = r.get("vgpr_count", 0) + r.get("agpr_count", 0)
            r["waves_per_simd"] = min(8, 512 // max(8, (regs + 7) // 8 * 8))
            rows.append(r)
    cols = [("kernel", "kernel"), ("waits<VL", "waits_before_first_vload"), ("br<VL", "branches_before_first_vload"),
            ("streams", "streams"), ("vm-between", "wait_or_branch_between_streams"),
            ("state<VL", "state_loads_before_first_vload"), ("VL..state", "waits_first_stream_to_last_state_load"), ("sqrt raw", "sqrt_raw"), ("sqrt corr", "sqrt_corrected"),
            ("insns", "instructions"), ("vgpr", "vgpr_count"), ("agpr", "agpr_count"), ("sgpr", "sgpr_count"),
            ("vspill", "vgpr_spill_count"), ("scratch", "private_segment_fixed_size"), ("lds", "group_segment_fixed_size"),
            ("waves", "waves_per_simd")]
    if md:
        print("| " + " | ".join(c for c, _ in cols) + " |")
        print("|" + "---|" * len(cols))
        for r in rows:
            print("| " + " | ".join(("`%s`" % r[k]) if c == "kernel" else str(r.get(k, "?")) for c, k in cols) + " |")
    else:
        for r in rows:
            print("  ".join("%s=%s" % (c, r.get(k, "?")) for c, k in cols))


if __name__ == "__main__":
    main()
