#!/usr/bin/env python3
"""Which of the compiled kernels does the GPU suite launch?  Writes the record profiles/coverage/kernels.txt.

The library picks its kernel at run time from a family of template instantiations (dockauv_device.h: select_step,
select_sequence; dockauv_policy.hip: launch_policy_forward), and one instantiation of a correct source can be wrong while its
siblings are exact (csrc/build.py: PER_SOURCE_FLAGS; profiles/r4/ab_same_box.txt).  This script joins

  * the compiled kernels: the function names in the resource-usage remarks of `python gym_dockauv_amd/csrc/build.py --usage`
    (--usage FILE: that command's output; without it the script runs the command), demangled with c++filt, and
  * the launched kernels: the Kernel_Name column of the kernel-trace CSVs that `rocprofv3 --kernel-trace --stats` wrote for the
    GPU suite, one traced run per test file or per test, each into a directory of its own under --traces:

      rocprofv3 --kernel-trace --stats --output-format csv -d traces/test_gpu_reset__test_step_sequence_equals_single_steps -- \\
          python -m pytest tests/test_gpu_reset.py -q -k test_step_sequence_equals_single_steps

    The directory's name is the label of everything launched below it ("__" stands for "::").

and prints one line per compiled kernel, `name launched|not-launched label(s)`, then the counts.  --notes FILE: lines
`<regular expression> | <text>` (the first " | " separates them); the text is put on every line whose kernel name the
expression matches and that no traced run launched (why nothing selects the kernel, which configuration would, or the tests
that launch it in child processes the tracer was not pointed at).

  python scripts/kernel_coverage.py --usage usage.txt --traces traces --notes profiles/coverage/notes.txt > profiles/coverage/kernels.txt

--previous FILE: a refresh from traced runs of some test files only -- a kernel that FILE (a copy of the earlier record) lists as
launched keeps that line's labels, with the labels of the new traces behind them.
"""
import argparse
import csv
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def demangle(names):
    names = list(names)
    if not names:
        return []
    out = subprocess.run(["c++filt"], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout
    return out.splitlines()


def normalise(name: str) -> str:
    """`void ns::kernel<args>(params) [clone .kd]` -> `kernel<args>`: what a remark's and a trace's spelling of one kernel share"""
    name = name.strip().strip('"')
    name = re.sub(r"\s*\[clone [^\]]*\]", "", name)
    if name.endswith(".kd"):
        name = name[:-3]
    name = name.replace("(anonymous namespace)::", "")
    if name.startswith("void "):
        name = name[5:]
    depth, cut = 0, len(name)
    for i, ch in enumerate(name):       # the parameter list opens at the first '(' outside the template arguments
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            cut = i
            break
    name = name[:cut]
    return re.sub(r"\bdockauv::", "", name).strip()   # (also inside template arguments: gae_kernel<dockauv::GaeArgs>)


def compiled_kernels(usage_text: str):
    mangled = sorted(set(re.findall(r"Function Name: (\S+)", usage_text)))
    return sorted(set(normalise(d) for d in demangle(mangled)))


def launched_kernels(traces_dir: str):
    """{kernel: sorted labels}; a label is the first directory below traces_dir"""
    found = {}
    for label in sorted(os.listdir(traces_dir)):
        top = os.path.join(traces_dir, label)
        if not os.path.isdir(top):
            continue
        for d, _, files in os.walk(top):
            for f in files:
                col = "Kernel_Name" if f.endswith("kernel_trace.csv") else ("Name" if f.endswith("kernel_stats.csv") else None)
                if col is None:
                    continue
                with open(os.path.join(d, f), newline="") as fh:
                    names = set(row[col] for row in csv.DictReader(fh) if row.get(col))
                mangled = [n for n in names if n.startswith("_Z")]
                names = (names - set(mangled)) | set(demangle(mangled))
                for n in names:
                    found.setdefault(normalise(n), set()).add(label.replace("__", "::"))
    return {k: sorted(v) for k, v in found.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--usage", help="output of `python gym_dockauv_amd/csrc/build.py --usage` (default: run it)")
    ap.add_argument("--traces", required=True, help="directory with one sub-directory of rocprofv3 output per traced run")
    ap.add_argument("--notes", help="file of `<regular expression> | <text>` lines for kernels no traced run launched")
    ap.add_argument("--previous", help="an earlier record: the labels of its `launched` lines are kept for kernels that this call's "
                                       "traces do not show (a refresh with traced runs of some test files only)")
    args = ap.parse_args()
    if args.usage:
        usage = open(args.usage).read()
    else:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "gym_dockauv_amd", "csrc", "build.py"), "--usage"],
                           capture_output=True, text=True, check=True)
        usage = r.stdout + r.stderr
    compiled = compiled_kernels(usage)
    launched = launched_kernels(args.traces)
    if args.previous:   # (a record's label text is kept as it stands -- some lines carry remarks -- and new labels go behind it)
        for line in open(args.previous):
            m = re.match(r"^([^#].*?) (not-launched|launched) (.+)$", line.rstrip("\n"))
            if m and m.group(2) == "launched":
                new = [lab for lab in launched.get(m.group(1), []) if lab not in m.group(3).split()]
                launched[m.group(1)] = [m.group(3)] + new
    notes = []
    if args.notes:
        for line in open(args.notes):
            if " | " in line and not line.startswith("#"):
                key, text = line.split(" | ", 1)
                notes.append((key.strip(), text.strip()))
    n_launched = n_noted = 0
    family = {}
    for k in compiled:
        fam = family.setdefault(k.split("<")[0], [0, 0])
        fam[1] += 1
        if k in launched:
            n_launched += 1
            fam[0] += 1
            print(f"{k} launched {' '.join(launched[k])}")
        else:
            text = "; ".join(t for key, t in notes if re.search(key, k))
            n_noted += bool(text)
            print(f"{k} not-launched {text or '-'}")
    stray = sorted(k for k in launched if k not in compiled and not k.startswith(("at::", "void at::", "Cijk", "__amd")))
    print(f"# compiled {len(compiled)}, launched by a traced test {n_launched}, not launched {len(compiled) - n_launched} "
          f"(with a note {n_noted}, without {len(compiled) - n_launched - n_noted})")
    for fam, (a, b) in sorted(family.items()):
        print(f"# {fam}: {a} of {b} launched")
    own = [k for k in stray if "dockauv" in k or k.split("<")[0] in family]
    if own:
        print("# launched but not in the usage remarks: " + ", ".join(own))


if __name__ == "__main__":
    main()
