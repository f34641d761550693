#!/usr/bin/env python3
"""Registers and scalar-load round trips of every float step-kernel instantiation, from the ISA (cross-compiles, no GPU).

usage: python scripts/scalar_round_trips.py [--keep DIR] [-DFLAG ...]      > profiles/hot_params/kernel_usage_<what>.txt
       python scripts/scalar_round_trips.py --diff BEFORE.txt AFTER.txt     (the guard rails of DESIGN.md section 3)

The float32 and the resident-sequence translation units are compiled with the flags of gym_dockauv_amd/csrc/build.py plus
`--cuda-device-only -S -Rpass-analysis=kernel-resource-usage`.  Per kernel:
  vgpr, sgpr-spill, scratch   from the resource-usage remarks
  s_load                      scalar loads in the kernel
  trips                       round trips, whole kernel: an `s_waitcnt` with lgkmcnt(0) that retires at least one scalar load
                              issued since the previous such wait
  trips-env                   round trips between the first vector load and the fifth right-hand side, in layout order: from
                              the first `global_load` to the fifth `v_rcp_f32` behind it (rhs_ divides by cos(theta) once and
                              nothing in front of the stages divides; the mixed kernels lay out two vehicle models: the tenth)
  trips-tail                  round trips behind the integrator, in layout order: from that fifth (mixed: tenth) `v_rcp_f32` to the
                              first `s_endpgm` behind it
Only `s_load*`, `s_waitcnt`, `global_load*`, `v_rcp_f32` and `s_endpgm` are looked at."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gym_dockauv_amd.csrc import build as hip_build  # noqa: E402

UNITS = ["dockauv_kernels_f32.hip", "dockauv_kernels_seq.hip"]
VK = {0: "BlueROV2", 1: "denseB", 2: "LAUV", 3: "mixed"}


def compile_units(folder, extra):
    flags = [f for f in hip_build.FLAGS if f not in ("-shared", "-fPIC")]
    procs = []
    for src in UNITS:
        s = os.path.join(folder, src.replace(".hip", ".s"))
        cmd = [hip_build.HIPCC, *flags, *extra, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", s]
        procs.append((s, subprocess.Popen(cmd, cwd=hip_build.HERE, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    out = []
    for s, p in procs:
        remarks, _ = p.communicate()
        if p.returncode != 0:
            sys.stderr.write(remarks)
            raise SystemExit("hipcc failed")
        out.append((open(s).read(), remarks))
    return out


def count_trips(lines):
    trips, pending = 0, 0
    for op, rest in lines:
        if op.startswith("s_load") or op.startswith("s_buffer_load"):
            pending += 1
        elif op == "s_waitcnt" and "lgkmcnt(0)" in rest:
            if pending:
                trips += 1
            pending = 0
    return trips


def analyse(asm, remarks):
    rows = []
    for nm in re.findall(r"\n(_ZN7dockauv\d+step_(?:seq_|ride_)?kernel\w+):", asm):
        dem = subprocess.run(["c++filt", nm], capture_output=True, text=True).stdout.strip()
        m = re.search(r"(step_\w*kernel)<float, (\d), (\w+), (\w+), 64, (\d+)((?:, \w+)*)>", dem)
        if not m:
            continue
        kind, vk, sym, rays, nt = m.group(1), int(m.group(2)), m.group(3) == "true", m.group(4) == "true", int(m.group(5))
        tail = [x == "true" for x in m.group(6).replace(",", " ").split()]
        log, term, wb = (tail + [False] * 3)[:3] if kind == "step_kernel" else (False, False, bool(tail and tail[0]))
        body = asm.split("\n" + nm + ":")[1].split(".Lfunc_end")[0]
        lines = []
        for ln in body.split("\n"):
            if ln.startswith("\t") and not ln.strip().startswith((";", ".")):
                parts = ln.strip().split(None, 1)
                lines.append((parts[0], parts[1] if len(parts) > 1 else ""))
        first = next((i for i, (op, _) in enumerate(lines) if op.startswith("global_load")), None)
        env = tail = "-"
        if first is not None:
            need, seen, end = (10 if vk == 3 else 5), 0, None
            for i in range(first, len(lines)):
                if lines[i][0] == "v_rcp_f32_e32" or lines[i][0] == "v_rcp_f32":
                    seen += 1
                    if seen == need:
                        end = i
                        break
            if end is not None:
                env = str(count_trips(lines[first:end]))
                stop = next((i for i in range(end, len(lines)) if lines[i][0] == "s_endpgm"), len(lines))
                tail = str(count_trips(lines[end:stop]))
        u = re.search(re.escape(nm) + r".*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+)", remarks, re.S)
        vg, scr, ssp = u.groups() if u else ("?",) * 3
        what = "full" if log else ("term" if term else ("wb" if wb else "plain"))
        name = f"{kind:16s} {VK[vk]:8s} sym={int(sym)} rays={int(rays)} threads={nt:3d} {what:5s}"
        n_load = sum(1 for op, _ in lines if op.startswith("s_load"))
        rows.append((kind, not sym, log, vk, not rays, -nt, what,
                     f"{name} | vgpr {vg:>3s} sgpr-spill {ssp:>3s} scratch {scr:>3s} | s_load {n_load:3d} trips {count_trips(lines):3d} trips-env {env:>3s} trips-tail {tail:>3s}"))
    return rows


def diff(before, after):
    def table(path):
        t = {}
        for ln in open(path):
            if "|" in ln:
                v = [int(x) if x.isdigit() else None for x in re.findall(r"(?:vgpr|sgpr-spill|scratch|trips|trips-env|trips-tail) +(\S+)", ln)]
                t[ln.split("|")[0].strip()] = (v + [None])[:6]   # (tables older than the trips-tail column)
        return t
    b, a = table(before), table(after)
    bad = 0
    for k in sorted(a):
        if k not in b:
            print(f"{k}: new")
            continue
        (v0, s0, c0, t0, e0, l0), (v1, s1, c1, t1, e1, l1) = b[k], a[k]
        broken = (v1 > 128) or (c1 > c0) or (s1 > s0)
        bad += broken
        if broken or (v0, s0, c0, t0, e0, l0) != (v1, s1, c1, t1, e1, l1):
            print(f"{k}: vgpr {v0} -> {v1}, sgpr-spill {s0} -> {s1}, scratch {c0} -> {c1}, trips {t0} -> {t1}, trips-env {e0} -> {e1}, "
                  f"trips-tail {l0} -> {l1}" + ("   ** GUARD RAIL **" if broken else ""))
    print(f"{len(a)} kernels, {bad} over a guard rail (VGPRs <= 128, no scratch added, no more SGPR spills)")
    return bad


def main():
    args = sys.argv[1:]
    if args and args[0] == "--diff":
        raise SystemExit(1 if diff(args[1], args[2]) else 0)
    keep = None
    if args and args[0] == "--keep":
        keep, args = args[1], args[2:]
        os.makedirs(keep, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        units = compile_units(keep or tmp, args)
    print("kernel<float, vehicle, SYM, RAYS, 64, threads, ...>: registers, scalar loads and round trips (scripts/scalar_round_trips.py)")
    rows = []
    for asm, remarks in units:
        rows += analyse(asm, remarks)
    for r in sorted(rows):
        print(r[-1])


if __name__ == "__main__":
    main()
