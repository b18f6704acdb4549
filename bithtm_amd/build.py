"""Build libbithtm_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""

import json
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libbithtm_hip.so")
RESOURCES = os.path.join(HERE, "libbithtm_hip.resources.json")     # what the compiler gave every kernel (written beside the library)
# Features added after the classifier banks report their kernels into a file of their own, keyed by the header that defines them:
# tests/test_group_classifier_cpu.py holds the set of kernels in RESOURCES to what it was with the banks, and a feature's own test
# holds its kernels' figures (kernel_resources("htm_knn.h"): tests/test_knn_cpu.py).  all_kernel_resources() is every kernel of the library.
OWN_REPORTS = {"htm_knn.h": os.path.join(HERE, "libbithtm_hip.knn.resources.json")}
# ... and kernels added later still, whose reports all_kernel_resources() -- held to RESOURCES + OWN_REPORTS by tests/test_knn_cpu.py -- does
# not return either: every_kernel_resources() is every kernel of the library (tests/test_handover_cpu.py).
LATER_REPORTS = {"htm_handover.h": os.path.join(HERE, "libbithtm_hip.handover.resources.json")}
# ... and the banks of KNN classifiers, which none of the three functions above returns (tests/test_handover_cpu.py holds
# every_kernel_resources() to the three reports it had): library_kernel_resources() is every kernel of the library.
BANK_REPORTS = {"htm_knn_bank.h": os.path.join(HERE, "libbithtm_hip.knn_bank.resources.json")}
# ... and the last launch of the batched run's two-launch step with its list role, which none of the four functions above returns
# (tests/test_group_knn_cpu.py holds library_kernel_resources() to the four reports it had): whole_library_kernel_resources() is every
# kernel of the library (tests/test_winner_list_cpu.py).
LAST_REPORTS = {"htm_handover_last.h": os.path.join(HERE, "libbithtm_hip.handover_last.resources.json")}
# ... and the coordinate fields' kernels, which none of the five functions above returns (tests/test_winner_list_cpu.py holds
# whole_library_kernel_resources() to the five reports it had): kernel_resources("htm_coord.h") (tests/test_coordinate_cpu.py).
COORD_REPORTS = {"htm_coord.h": os.path.join(HERE, "libbithtm_hip.coord.resources.json")}
# ... and the pooling links' kernels, which none of the five functions above returns either: kernel_resources("htm_pool.h")
# (tests/test_pooling_cpu.py).
POOL_REPORTS = {"htm_pool.h": os.path.join(HERE, "libbithtm_hip.pool.resources.json")}
# ... and the member-indexed link kernels of stacks of model groups: kernel_resources("htm_group_stack.h")
# (tests/test_group_stack_cpu.py).
GROUP_STACK_REPORTS = {"htm_group_stack.h": os.path.join(HERE, "libbithtm_hip.group_stack.resources.json")}
SOURCES = ["htm_engine.hip"]
HEADERS = ["htm_dev.h", "htm_sp_kernels.h", "htm_tm_kernels.h", "htm_pipeline.h", "htm_record.h", "htm_reset.h", "htm_decode.h", "htm_stack.h", "htm_pool.h", "htm_pool_select.inc", "htm_group_stack.h", "htm_forecast.h", "htm_noise.h", "htm_group.h", "htm_tm_feed.h", "htm_sp_run.h", "htm_fork.h", "htm_scalar.h", "htm_live.h", "htm_fields.h", "htm_coord.h", "htm_likelihood.h", "htm_classifier.h", "htm_knn.h", "htm_knn_bank.h", "htm_handover.h", "htm_handover_last.h", "htm_rng.h", "htm_fexp.h",
           os.path.join("..", "..", "include", "bithtm_hip.h")]
# -ffp-contract=off: several kernels must round exactly like the NumPy expressions they replace
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
         "-fno-fast-math", "-Wall", "-Wno-unused-result", "-Wno-unused-value",
         "-Rpass-analysis=kernel-resource-usage"]


def _stale():
    if not os.path.exists(LIB) or not all(os.path.exists(r) for r in [RESOURCES] + list(OWN_REPORTS.values()) + list(LATER_REPORTS.values()) + list(BANK_REPORTS.values()) + list(LAST_REPORTS.values()) + list(COORD_REPORTS.values()) + list(POOL_REPORTS.values()) + list(GROUP_STACK_REPORTS.values())):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS] + [os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > t for d in deps)


def _kernel_resources(log):
    """The compiler's per-kernel remarks -> {mangled name: {"vgprs", "agprs", "sgprs", "scratch_bytes_per_lane", "occupancy",
    "lds_bytes"}} per header that defines the kernel: {header file name: {...}}.  k_learn_scan_emit lives at 80 VGPRs (6 waves per SIMD) with NO scratch: a single spilled register slows
    every role of that launch by microseconds (LABNOTES.md) -- tests/test_host_and_abi.py holds the build to it."""
    fields = {"VGPRs": "vgprs", "AGPRs": "agprs", "SGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
              "Occupancy [waves/SIMD]": "occupancy", "LDS Size [bytes/block]": "lds_bytes"}
    out, cur = {}, None
    for line in log.splitlines():
        m = re.search(r"^(?:(\S+?):\d+:\d+: )?remark: +([^:]+): (\S+) \[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        key, val = m.group(2).strip(), m.group(3)
        if key == "Function Name":
            cur = out.setdefault(os.path.basename(m.group(1) or ""), {}).setdefault(val, {})
        elif cur is not None and key in fields:
            cur[fields[key]] = int(val)
    return out


def _without_remarks(log):
    """The compiler's output minus the resource remarks (each with its `In file included from` chain and source snippet)."""
    out, pending, in_remark = [], [], False
    for line in log.splitlines():
        if "kernel-resource-usage" in line:
            pending, in_remark = [], True
        elif line.startswith("In file included from"):
            pending.append(line)
            in_remark = False
        elif in_remark and re.match(r"\s*\d*\s*\|", line):
            continue
        else:
            out += pending + [line]
            pending, in_remark = [], False
    return "\n".join(out)


def build(force=False, verbose=False):
    if not force and not _stale():
        return LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    extra = os.environ.get("BITHTM_EXTRA_FLAGS", "").split()      # diagnostic builds (e.g. -DBITHTM_LEARN_STAMPS)
    cmd = [hipcc] + FLAGS + extra + [os.path.join(CSRC, s) for s in SOURCES] + ["-o", LIB]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + r.stdout)
    by_header = _kernel_resources(r.stdout)
    for header, path in list(OWN_REPORTS.items()) + list(LATER_REPORTS.items()) + list(BANK_REPORTS.items()) + list(LAST_REPORTS.items()) + list(COORD_REPORTS.items()) + list(POOL_REPORTS.items()) + list(GROUP_STACK_REPORTS.items()):
        with open(path, "w") as f:
            json.dump(by_header.pop(header, {}), f, indent=0, sort_keys=True)
    with open(RESOURCES, "w") as f:
        json.dump({k: v for kernels in by_header.values() for k, v in kernels.items()}, f, indent=0, sort_keys=True)
    if verbose:
        rest = _without_remarks(r.stdout)
        if rest.strip():
            print(rest, file=sys.stderr)
    return LIB


def kernel_resources(header=None):
    """{mangled kernel name: resources} of the library as last built here (None if it was built elsewhere): the kernels of RESOURCES,
    or those the header `header` of OWN_REPORTS, LATER_REPORTS, BANK_REPORTS, LAST_REPORTS, COORD_REPORTS, POOL_REPORTS or GROUP_STACK_REPORTS defines."""
    build()
    path = RESOURCES if header is None else {**OWN_REPORTS, **LATER_REPORTS, **BANK_REPORTS, **LAST_REPORTS, **COORD_REPORTS, **POOL_REPORTS, **GROUP_STACK_REPORTS}[header]
    if not os.path.exists(path):
        return None
    with open(path) as f:
        return json.load(f)


def all_kernel_resources():
    """RESOURCES and the reports of OWN_REPORTS together (None if it was built elsewhere): every kernel the library had with the KNN
    classifier.  The kernels of LATER_REPORTS are not among them: every_kernel_resources()."""
    parts = [kernel_resources()] + [kernel_resources(h) for h in OWN_REPORTS]
    return None if any(p is None for p in parts) else {k: v for p in parts for k, v in p.items()}


def every_kernel_resources():
    """Every kernel of the library: all_kernel_resources() and the reports of LATER_REPORTS together (None if it was built elsewhere)."""
    parts = [all_kernel_resources()] + [kernel_resources(h) for h in LATER_REPORTS]
    return None if any(p is None for p in parts) else {k: v for p in parts for k, v in p.items()}


def library_kernel_resources():
    """Every kernel the library had with the KNN classifier banks: every_kernel_resources() and the reports of BANK_REPORTS together
    (None if it was built elsewhere).  The kernels of LAST_REPORTS are not among them: whole_library_kernel_resources()."""
    parts = [every_kernel_resources()] + [kernel_resources(h) for h in BANK_REPORTS]
    return None if any(p is None for p in parts) else {k: v for p in parts for k, v in p.items()}


def whole_library_kernel_resources():
    """Every kernel of the library: library_kernel_resources() and the reports of LAST_REPORTS together (None if it was built elsewhere)."""
    parts = [library_kernel_resources()] + [kernel_resources(h) for h in LAST_REPORTS]
    return None if any(p is None for p in parts) else {k: v for p in parts for k, v in p.items()}


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
