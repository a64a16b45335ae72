"""Static check of the hand-issued LDS reads of the float64 kernels (xcorr_f64_split.hpp, xcorr_f64.hip).

Those kernels issue `ds_read_b64 / ds_read_b128` through inline asm and wait for them with a separate counted
`s_waitcnt lgkmcnt(N)` asm statement, so that the next batch of reads is in flight while the current one is consumed.  The
compiler's own wait-count insertion does not see inline asm: nothing but the data dependency through the wait statement
tells it that the destination registers are not valid yet.  If it ever copied, spilled or otherwise READ such a register
between the read and the wait that covers it, the kernel would silently use stale data.  This script compiles
the translation unit to assembly and walks every kernel: LDS operations are kept in issue order (the LDS returns in order),
`s_waitcnt lgkmcnt(N)` retires all but the N youngest, and any instruction that names a register of a read still in flight
is reported.

    python tools/check_lds_inflight.py [xcorr_f64]      -> exit code 1 and the offending lines if the constraint is broken

Second check (half_barriers): the 64 x 64 float64 kernels instantiate their whole window loop once per line half behind ONE
wave-uniform branch at the top (TPIV_F64_PER_HALF, xcorr_f64.hip).  The two wavefronts of a workgroup then run DIFFERENT
code and meet at workgroup barriers, so both copies must execute the same number of s_barrier per window or the workgroup
hangs.  The walk splits the kernel at its first scalar-condition branch -- copy 0 up to the branch's target, copy 1 from
there to s_endpgm --, takes the widest backward-branch span of each copy as its window loop and counts the s_barrier
INSTRUCTIONS in it.  That is a static count: a barrier inside a conditional block (the val_win > 4 zone path) counts as if
always executed, one inside an inner loop counts once.  Equal static counts are necessary for equal executed counts, not
sufficient; what the check catches is a copy that gained or lost a barrier instruction.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-std=c++17", "-O3", "-fPIC", "-ffp-contract=fast-honor-pragmas", "-fno-slp-vectorize",
         "-mllvm", "-amdgpu-atomic-optimizer-strategy=None", "-Wno-unused-result", "-S", "--cuda-device-only"]


def regs(tok):
    m = re.match(r"-?\|?v\[(\d+):(\d+)\]\|?$", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"-?\|?v(\d+)\|?$", tok)
    return {int(m.group(1))} if m else set()


def check(asm_text):
    problems, n_reads = [], 0
    kernel, fifo = None, []                      # fifo: [registers written by the op (empty for stores / others)]
    in_asm = False                               # between ;;#ASMSTART and ;;#ASMEND: a hand-issued instruction
    for ln, line in enumerate(asm_text.splitlines(), 1):
        if "#ASMSTART" in line:
            in_asm = True
        elif "#ASMEND" in line:
            in_asm = False
        s = line.split(";")[0].strip()
        if not s:
            continue
        m = re.match(r"^(_Z\w+):", s)
        if m:
            kernel, fifo = m.group(1), []
            continue
        if s.endswith(":") or s.startswith("."):
            continue
        parts = s.split(None, 1)
        op = parts[0]
        toks = [t.strip().split(" ")[0] for t in parts[1].split(",")] if len(parts) > 1 else []
        if op == "s_waitcnt":
            m = re.search(r"lgkmcnt\((\d+)\)", s)
            if m:
                keep = int(m.group(1))
                fifo = fifo[len(fifo) - keep:] if keep else []
            continue
        if op in ("s_barrier", "s_endpgm") or op.startswith("s_cbranch") or op == "s_branch":
            # (control flow: the kernels wait for lgkmcnt(0) in front of every barrier; across branches the walk is linear,
            #  which is conservative enough for straight-line read batches)
            continue
        used = set().union(*[regs(t) for t in toks]) if toks else set()
        inflight = set().union(*fifo) if fifo else set()
        if op.startswith("ds_read") or op.startswith("ds_load"):
            dst = regs(toks[0]) if toks else set()
            if (used - dst) & inflight or dst & inflight:
                problems.append((kernel, ln, line.strip()))
            # only the hand-issued reads are at risk: the compiler waits for its own reads before it touches their registers
            fifo.append(dst if in_asm else set())
            n_reads += in_asm
            continue
        if op.startswith("ds_") or op.startswith("s_load") or op.startswith("s_buffer_load"):
            if used & inflight:
                problems.append((kernel, ln, line.strip()))
            fifo.append(set())
            continue
        if used & inflight:
            problems.append((kernel, ln, line.strip()))
    return problems, n_reads


def kernel_bodies(asm_text):
    """{mangled kernel name: its lines, up to and including s_endpgm's block}"""
    out, name = {}, None
    for line in asm_text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            name = None
        if name is not None:
            out[name].append(line)
    return out


def reads_by_kernel(asm_text):
    """{kernel: (problems, hand-issued reads walked)} -- check() on each kernel's own lines."""
    return {k: check("\n".join(v)) for k, v in kernel_bodies(asm_text).items()}


PER_HALF_KERNELS = ("xcorr_f64_split_kernelILi64E", "xcorr_f64_list_kernelILi64E")      # TPIV_F64_PER_HALF instances (xcorr_f64.hip)


def half_barriers(lines):
    """-> [s_barrier per window-loop iteration in copy 0, in copy 1] of a kernel whose body is instantiated twice behind one
    wave-uniform branch at the top, or None where the body has no such branch."""
    ops = []                                  # (kind, argument): label / branch / barrier / end, in program order
    for line in lines:
        s = line.split(";")[0].strip()
        if not s:
            continue
        m = re.match(r"^(\.LBB\w+):", s)
        if m:
            ops.append(("label", m.group(1)))
            continue
        op = s.split()[0]
        if op == "s_barrier":
            ops.append(("barrier", None))
        elif op == "s_endpgm":
            ops.append(("end", None))
        elif op.startswith("s_cbranch") or op == "s_branch":
            ops.append((op, s.split()[-1]))
    first = next((i for i, (k, _) in enumerate(ops) if k.startswith("s_cbranch_scc")), None)
    if first is None:
        return None
    where = {a: i for i, (k, a) in enumerate(ops) if k == "label"}
    split = where.get(ops[first][1])
    end = next((i for i, (k, _) in enumerate(ops) if k == "end"), len(ops))
    if split is None or not first < split < end:
        return None
    counts = []
    for lo, hi in ((first + 1, split), (split, end)):
        spans = [(where[a], i) for i, (k, a) in enumerate(ops[:hi]) if i >= lo and k.startswith("s_") and k != "s_barrier"
                 and a in where and lo <= where[a] < i]
        if not spans:
            counts.append(0)
            continue
        a, b = max(spans, key=lambda ab: ab[1] - ab[0])
        counts.append(sum(1 for k, _ in ops[a:b] if k == "barrier"))
    return counts


def compile_asm(unit, extra=()):
    src = os.path.join(ROOT, "torchpiv_amd", "csrc", unit + ".hip")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, unit + ".s")
        subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, *extra, src, "-o", out], check=True, stderr=subprocess.DEVNULL)
        return open(out).read()


def per_half_report(asm_text):
    """{per-half kernel: [barriers in copy 0, in copy 1]} of the shipped per-half instances."""
    return {k: half_barriers(v) for k, v in kernel_bodies(asm_text).items() if any(t in k for t in PER_HALF_KERNELS)}


def main(unit="xcorr_f64"):
    text = compile_asm(unit)
    problems, n_reads = check(text)
    for k, c in per_half_report(text).items():
        print(f"{k}: s_barrier per window in the two per-half copies: {c}")
        if c is None or c[0] != c[1] or c[0] == 0:
            problems.append((k, 0, f"per-half copies disagree on their barriers: {c}"))
    print(f"{unit}: {n_reads} hand-issued LDS reads walked, {len(problems)} problem(s): a register used while its read is in flight, "
          f"or per-half copies with different barrier counts")
    for k, ln, text in problems[:20]:
        print(f"  {k} line {ln}: {text}")
    return 1 if problems else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:]))
