"""Build-time ISA check of the HEADS of the latency-bound Krylov kernels (csrc/device_utils.h: partials_request / partials_fold, pin_args, CtlHead;
profiles/krylov_heads.txt).  These kernels move next to no data; their time is a chain of dependent memory trips, and how many trips the head takes is
decided by where the compiler puts its waits, not by the order of the loads in the source.  On the code objects of both libraries, for
k_cg_dirMs<3, 2>, k_cg_updF<2> (both halves), k_cg_upd<false> and k_fold_start<false>, along the cheapest path from the kernel's entry to its first
s_barrier (cheapest = fewest full drains, then fewest argument groups: the path of a regular iteration; the paths of an expected no-op launch and of
an operator without the tile-major copy are longer):

  * full drains of the vector memory counter, `s_waitcnt vmcnt(0)` with at least one vector load issued on the path since the previous one;
  * groups of kernel-argument loads (s_load from s[0:1]) that are separated by a wait on the scalar counter;

and, in program order, that no wait of any kind stands between the first and the last load of a thread's eight reduction partials.

The build before this test had, in every one of these kernels, the first partial's load drained on the spot (the other seven were issued behind that
drain) and three to five argument groups; the figures are next to PARENT below."""
import glob
import heapq
import os
import re
import shutil
import subprocess

import pytest

import cosmo_jl_amd as cj

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"

# kernel -> (mangled prefix, halves, {dtype: (drains, argument groups) the build reaches per half}); a half = a successor of the kernel's first conditional
# branch (k_cg_updF: vector update / dense-row tiles, in either order)
KERNELS = {
    "k_cg_dirMs<3, 2>": ("_Z10k_cg_dirMsILi3ELi2EE", 1),
    "k_cg_updF<2>": ("_Z9k_cg_updFILi2EE", 2),
    "k_cg_upd<false>": ("_Z8k_cg_updILb0EE", 1),
    "k_fold_start<false>": ("_Z12k_fold_startILb0EE", 1),
}
# (drains, argument groups) of the build before, as THIS test counts them on its libraries (cheapest path; both precisions alike): 2 / 5 in k_cg_dirMs<3, 2>,
# 2 / 3 in each half of k_cg_updF<2>, 2 / 4 in k_cg_upd<false>, 0 / 3 in k_fold_start<false> (one workgroup folds partials there, off the cheapest path).
# Counted in program order over all blocks (every drain the listing shows) the same build has 3 / 4 and 2 / 3 in the first two.  The new values must be
# BELOW the smaller of the two counts.
PARENT = {"k_cg_dirMs<3, 2>": (2, 4), "k_cg_updF<2>": (2, 3), "k_cg_upd<false>": (2, 4)}
REACHED = {                                                              # what this build reaches (per half): a regression fails, an improvement passes
    "float64": {"k_cg_dirMs<3, 2>": [(1, 1)], "k_cg_updF<2>": [(1, 1), (1, 1)], "k_cg_upd<false>": [(1, 1)], "k_fold_start<false>": [(0, 1)]},
    "float32": {"k_cg_dirMs<3, 2>": [(1, 1)], "k_cg_updF<2>": [(1, 1), (1, 1)], "k_cg_upd<false>": [(1, 1)], "k_fold_start<false>": [(0, 1)]},
}


def disassemble(lib, work):
    """-> {function name: [(address, opcode, operand text, branch target address or None)]} over all gfx950 code objects of the library"""
    local = os.path.join(work, os.path.basename(lib))
    shutil.copy(lib, local)                                            # (--offloading writes the extracted bundles NEXT TO its input)
    subprocess.run([OBJDUMP, "--offloading", local], cwd=work, capture_output=True, text=True, check=True)
    cos = sorted(glob.glob(os.path.join(work, "*hipv4-amdgcn-amd-amdhsa--gfx950")))
    assert len(cos) >= 10, cos
    fns = {}
    for co in cos:
        out = subprocess.run([OBJDUMP, "-d", co], capture_output=True, text=True, check=True).stdout
        fn, base = None, 0
        for ln in out.splitlines():
            m = re.match(r"^([0-9a-f]+) <(.+)>:", ln)
            if m:
                base, fn = int(m.group(1), 16), m.group(2)
                fns[fn] = []
                continue
            if fn is None or "//" not in ln:
                continue
            text, comment = ln.split("//", 1)
            text = text.strip()
            ma = re.match(r"\s*([0-9A-Fa-f]+):", comment)
            if not text or not ma:
                continue
            op = text.split()[0]
            target = None
            if op.startswith("s_cbranch") or op == "s_branch":
                mt = re.search(r"<.+\+0x([0-9a-fA-F]+)>", comment)
                target = base + int(mt.group(1), 16) if mt else base
            fns[fn].append((int(ma.group(1), 16), op, text, target))
    return fns


def _is_drain(op, text):
    return op == "s_waitcnt" and "vmcnt(0)" in text


def _is_arg_load(op, text):
    return op.startswith("s_load") and re.search(r",\s*s\[0:1\]\s*,", text) is not None


def _is_vload(op):
    return op.startswith(("global_load", "buffer_load", "flat_load", "scratch_load"))


def cheapest_head(ins, start, state=(0, 0, False, False)):
    """Fewest (drains, argument groups) from instruction index `start` to the first s_barrier, over all paths; None if no path reaches one."""
    index = {a: i for i, (a, _, _, _) in enumerate(ins)}
    heap = [(state[0], state[1], start, state[2], state[3])]
    seen = set()
    while heap:
        dr, gr, i, ing, vm = heapq.heappop(heap)             # ing: inside a group of argument loads; vm: vector loads in flight
        if (i, ing, vm) in seen or i >= len(ins):
            continue
        seen.add((i, ing, vm))
        _, op, text, target = ins[i]
        if op == "s_barrier":
            return dr, gr
        if op == "s_endpgm":
            continue
        if _is_vload(op):
            vm = True
        if _is_drain(op, text):
            dr += 1 if vm else 0
            vm = False
        if op == "s_waitcnt" and "lgkmcnt" in text:
            ing = False
        if _is_arg_load(op, text):
            if not ing:
                gr += 1
            ing = True
        # a branch on EXEC skips a region no lane is active in (e.g. the parent's per-lane guarded partial loads): the region is part of the path
        if target is not None and target in index and not op.startswith("s_cbranch_exec"):
            heapq.heappush(heap, (dr, gr, index[target], ing, vm))
        if op != "s_branch":
            heapq.heappush(heap, (dr, gr, i + 1, ing, vm))
    return None


def entry_index(ins):
    """A kernel built with kernarg preloading (csrc/Makefile) starts with a 256-byte header for firmware without it -- s_load of the preloaded arguments, a wait,
    a branch over the padding; with preloading the packet processor starts the kernel BEHIND the header, with those arguments in SGPRs.  -> index of the entry."""
    base = ins[0][0]
    for i, (_, op, _, target) in enumerate(ins[:16]):
        if op == "s_branch" and target == base + 0x100 and all(o == "s_nop" for _, o, _, _ in ins[i + 1:i + 4]):
            return next(j for j, (a, _, _, _) in enumerate(ins) if a == base + 0x100)
    return 0


def heads(ins, halves):
    e = entry_index(ins)
    if halves == 1:
        return [cheapest_head(ins, e)]
    # the prefix up to the first conditional branch is common; each successor is a half
    dr = gr = 0
    ing = vm = False
    for i, (_, op, text, target) in enumerate(ins):
        if i < e:
            continue
        if op.startswith("s_cbranch"):
            idx = {a: j for j, (a, _, _, _) in enumerate(ins)}
            return [cheapest_head(ins, i + 1, (dr, gr, ing, vm)), cheapest_head(ins, idx[target], (dr, gr, ing, vm))]
        if _is_vload(op):
            vm = True
        if _is_drain(op, text):
            dr += 1 if vm else 0
            vm = False
        if op == "s_waitcnt" and "lgkmcnt" in text:
            ing = False
        if _is_arg_load(op, text):
            gr += 0 if ing else 1
            ing = True
    raise AssertionError("no conditional branch")


def partial_load_runs(ins, f32):
    """Runs of eight loads of a thread's partials: real-sized global loads off one scalar base, eight or more of them in the kernel, in program order.
    -> list of (number of s_waitcnt between the first and the last load of the run)."""
    opname = "global_load_dword" if f32 else "global_load_dwordx2"
    by_base = {}
    for i, (_, op, text, _) in enumerate(ins):
        if op == opname:
            m = re.search(r",\s*(s\[\d+:\d+\])", text)
            if m:
                by_base.setdefault(m.group(1), []).append(i)
    runs = []
    for base, idx in by_base.items():
        if len(idx) < 8:
            continue
        for k in range(0, len(idx) - 7, 8):
            a, b = idx[k], idx[k + 7]
            runs.append(sum(1 for j in range(a, b) if ins[j][1] == "s_waitcnt"))
    return runs


@pytest.mark.parametrize("which", ["float64", "float32"])
def test_heads_of_the_krylov_kernels(which, tmp_path):
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump of the ROCm toolchain not available")
    lib = cj._ffi.LIB_PATH if which == "float64" else cj._ffi.LIB_PATH_F32
    work = tmp_path / "co"
    work.mkdir()
    fns = disassemble(lib, str(work))
    for name, (prefix, halves) in KERNELS.items():
        match = [f for f in fns if f.startswith(prefix)]
        assert len(match) == 1, (name, match)
        ins = fns[match[0]]
        got = sorted(heads(ins, halves))
        runs = partial_load_runs(ins, which == "float32")
        print("%s %s: (drains, argument groups) per half %s; waits inside the runs of partial loads %s" % (which, name, got, runs))
        assert None not in got, (name, got)
        assert len(runs) >= halves and all(r == 0 for r in runs), (name, runs)       # every partial load issued before the first wait
        for (dr, gr), (dr_max, gr_max) in zip(got, sorted(REACHED[which][name])):
            assert dr <= dr_max and gr <= gr_max, (name, got, REACHED[which][name])
        if name in PARENT:
            for dr, gr in got:
                assert dr < PARENT[name][0] and gr < PARENT[name][1], (name, got, PARENT[name])
