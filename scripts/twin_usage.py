#!/usr/bin/env python3
"""Guard rails of a twin-kernel change, from the device assembly of two trees (cross-compiles, no GPU).

usage: python scripts/twin_usage.py PARENT_CSRC NEW_CSRC TWIN_TAG       > profiles/<change>/kernel_usage.txt
  PARENT_CSRC / NEW_CSRC: the gym_dockauv_amd/csrc folders of the parent checkout and of this tree
  TWIN_TAG: what the new kernels carry in their names where their twins carry TWIN_OF (default: nocap / nocur)

Both trees' float32 and resident-sequence translation units are compiled with the build's flags plus
`--cuda-device-only -S -Rpass-analysis=kernel-resource-usage`.
 1. Every kernel of the parent must compile to the code it had: bodies compared instruction for instruction (basic-block labels
    renumbered, comments and directives dropped), remarks value for value.
 2. Every new kernel beside its twin: no more VGPRs, no scratch added, no more SGPR spills, the same LDS bytes, fewer instructions."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gym_dockauv_amd.csrc import build as hip_build  # noqa: E402

UNITS = ["dockauv_kernels_f32.hip", "dockauv_kernels_seq.hip"]
FIELDS = (("sgpr", r"SGPRs: (\d+)"), ("vgpr", r"VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
          ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("sspill", r"SGPRs Spill: (\d+)"), ("vspill", r"VGPRs Spill: (\d+)"),
          ("lds", r"LDS Size \[bytes/block\]: (\d+)"))


def compile_tree(csrc, out):
    flags = [f for f in hip_build.FLAGS if f not in ("-shared", "-fPIC")]
    procs = []
    for src in UNITS:
        s = os.path.join(out, src.replace(".hip", ".s"))
        cmd = [hip_build.HIPCC, *flags, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", s]
        procs.append((src, s, subprocess.Popen(cmd, cwd=csrc, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    units = {}
    for src, s, p in procs:
        remarks, _ = p.communicate()
        if p.returncode != 0:
            sys.stderr.write(remarks)
            raise SystemExit("hipcc failed on " + src)
        units[src] = kernels(open(s).read(), remarks)
    return units


def kernels(asm, remarks):
    """mangled name -> (demangled name, normalised instruction list, remark values)"""
    names = re.findall(r"\n(_ZN7dockauv\w+):", asm)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    out = {}
    for nm, d in zip(names, dem):
        if ".amdhsa_kernel " + nm not in asm:
            continue
        body = asm.split("\n" + nm + ":")[1].split("\n", 1)[1].split(".Lfunc_end")[0]
        ins, labels = [], {}
        for ln in body.split("\n"):
            t = ln.split(";")[0].strip()
            if not t or t.startswith("."):
                m = re.match(r"(\.LBB\w+):", t)
                if m:
                    labels[m.group(1)] = f"L{len(labels)}"
                    ins.append(m.group(1) + ":")
                continue
            ins.append(re.sub(r"\s+", " ", t))
        ins = [re.sub(r"\.LBB\w+", lambda m: labels.get(m.group(0), m.group(0)), i) for i in ins]
        u = re.search(r"Function Name: " + re.escape(nm) + r"\b(.*?)(?=Function Name:|\Z)", remarks, re.S)
        vals = {k: int(re.search(rx, u.group(1)).group(1)) for k, rx in FIELDS} if u else {}
        out[nm] = (d.strip(), ins, vals)
    return out


def mix(ins):
    ops = [i.split()[0] for i in ins if not i.endswith(":")]
    c = {"instr": len(ops)}
    c["valu"] = sum(o.startswith("v_") for o in ops)
    c["salu"] = sum(o.startswith("s_") for o in ops)
    c["loads"] = sum(o.startswith("global_load") for o in ops)
    c["stores"] = sum(o.startswith(("global_store", "global_atomic")) for o in ops)
    c["lds"] = sum(o.startswith("ds_") for o in ops)
    c["scratch"] = sum(o.startswith("scratch_") for o in ops)
    return c


def line(ins, vals):
    c = mix(ins)
    return (f"instr {c['instr']:4d} valu {c['valu']:4d} salu {c['salu']:4d} vmem {c['loads'] + c['stores']:3d} (loads {c['loads']} stores {c['stores']}) "
            f"lds {c['lds']:3d} scratch {c['scratch']} | vgpr {vals['vgpr']} sgpr {vals['sgpr']} scratch {vals['scratch']} B occ {vals['occ']} "
            f"sgpr-spill {vals['sspill']} vgpr-spill {vals['vspill']} LDS {vals['lds']} B")


def main():
    parent_csrc, new_csrc = sys.argv[1], sys.argv[2]
    tag = sys.argv[3] if len(sys.argv) > 3 else "nocap"
    twin_of = sys.argv[4] if len(sys.argv) > 4 else "nocur"
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        parent, new = compile_tree(parent_csrc, a), compile_tree(new_csrc, b)
    bad = 0
    print("1. Every kernel of the parent against the same kernel of this tree (instruction for instruction; remarks value for value)\n")
    fresh = []
    for src in UNITS:
        same = diff = 0
        for nm, (dem, ins, vals) in parent[src].items():
            if nm in new[src] and new[src][nm][1] == ins and new[src][nm][2] == vals:
                same += 1
            else:
                diff += 1
                print(f"   DIFFERENT: {dem}")
        added = [nm for nm in new[src] if nm not in parent[src]]
        fresh += [(src, nm) for nm in added]
        bad += diff
        print(f"   {src}: {len(parent[src])} kernels of the parent, {same} identical (instructions, registers, spills, scratch, LDS), {diff} different; "
              f"{len(added)} new kernels")
    print(f"\n2. The new ({tag}) kernels beside their twins ({twin_of}, same template arguments).  The rails: no more VGPRs, no scratch added,\n"
          "   no more SGPR spills, the same LDS bytes, fewer instructions.\n")
    for src, nm in fresh:
        dem, ins, vals = new[src][nm]
        twin = nm.replace(tag, twin_of)
        if twin not in new[src]:
            print(f"   new     {dem}\n     (no twin named {twin})")
            continue
        tdem, tins, tvals = new[src][twin]
        print(f"   new     {dem}\n            {line(ins, vals)}\n     twin   {line(tins, tvals)}")
        broken = []
        if vals["vgpr"] > tvals["vgpr"]: broken.append("more VGPRs")
        if vals["scratch"] > tvals["scratch"]: broken.append("more scratch")
        if vals["sspill"] > tvals["sspill"]: broken.append("more SGPR spills")
        if vals["vspill"] > tvals["vspill"]: broken.append("more VGPR spills")
        if vals["lds"] != tvals["lds"]: broken.append("other LDS bytes")
        if mix(ins)["instr"] >= mix(tins)["instr"]: broken.append("not fewer instructions")
        bad += bool(broken)
        print("     guard rails: " + ("OK" if not broken else "BROKEN: " + ", ".join(broken)))
    print(f"\n{'ALL RAILS HOLD' if not bad else str(bad) + ' PROBLEMS'}")
    return 1 if bad else 0


if __name__ == "__main__":
    raise SystemExit(main())
