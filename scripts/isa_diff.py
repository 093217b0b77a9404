"""Do two IPM kernel trees compile to the same code?  (CPU: compile and disassemble only.)  For every
structure in the kernel cache (populate it first, as scripts/lds_report.py assumes) the main,
-DMPCX_WS_LDS, -DMPCX_MIN_WAVES=1 and -DMPCX_APC=20 code objects are built against both include
directories (kernel trees as scripts/kernel_tree.py writes them) and compared: the ``llvm-objdump -d``
text without the line that names the file, and ``llvm-readelf --notes`` (the kernels' metadata: LDS,
registers, scratch).  The code objects' bytes are not compared: they differ between identical builds.
A build that fails must fail with the same error messages on both sides (a structure that does not
fit a variant fails the kernel's static_assert); that counts as equal.  One line per build:
``identical``, or the symbols whose bodies differ (call distances masked, so a caller of a function
that only moved is not listed) and whether the metadata differs.
``--diag``: also the diagnostic defines of the GPU tests, for the structures those tests use
(tests/test_gpu_ipm_fallbacks.py; the filter builds of tests/test_gpu_ipm.py).
usage: python scripts/isa_diff.py DIR_A DIR_B [--diag] [--jobs N]"""
import argparse
import concurrent.futures as cf
import os
import pathlib
import re
import subprocess
import sys
import tempfile

from lds_report import main_sources, native

SHIPPED = ((), ("MPCX_WS_LDS",), ("MPCX_MIN_WAVES=1",), ("MPCX_APC=20",))
LLVM = pathlib.Path(os.path.realpath(native._hipcc())).parents[1] / "llvm" / "bin"


def diag_builds(work):
    """(label, source, defines) of the GPU tests' diagnostic main builds."""
    from agentlib_mpc_amd import benchmarks as bm
    from tests import configs
    from tests import test_gpu_ipm_fallbacks as fb

    def src(name, gen):
        p = work / f"{name}.hip"
        p.write_text(gen.source)
        return p
    out = []
    for name in fb.CASES:
        s = src(name, configs.CASES[name]().backend.problem.gen)
        chain = ("MPCX_CHAIN_BK", "MPCX_CHAIN_SERIAL") if name in fb.CHAIN_CASES else ()
        out += [(name, s, (d,)) for d in ("MPCX_NO_STATIC", "MPCX_FORCE_BLOCK_CHAIN", *chain)]
    s = src("cubic_room", bm.cubic_room()[0].problem.gen)
    out += [("cubic_room", s, tuple(defs.split(","))) for defs, _cap in bm.FILTER_TEST_BUILDS.values()]
    return out


def compile_one(src, inc, defines, out):
    """-> ("ok", disassembly lines, notes) or ("failed", error messages, "")."""
    cmd = [native._hipcc(), "--genco", "--no-gpu-bundle-output", f"--offload-arch={native.OFFLOAD_ARCH}", "-O3",
           "-std=c++17", f"-I{inc}", f"-I{native.INCLUDE}", f"-I{native.CSRC}", *[f"-D{d}" for d in defines],
           str(src), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return "failed", sorted(set(re.findall(r"error: (.*)", r.stderr))) or [r.stderr[-300:]], ""
    dis = subprocess.run([LLVM / "llvm-objdump", "-d", str(out)], capture_output=True, text=True, check=True).stdout
    notes = subprocess.run([LLVM / "llvm-readelf", "--notes", str(out)], capture_output=True, text=True, check=True).stdout
    out.unlink()
    notes = "\n".join(ln for ln in notes.splitlines() if "NT_AMDGPU_METADATA" not in ln)  # the note's size
    lines = dis.splitlines()
    assert str(out) in "\n".join(lines[:3]), lines[:3]
    return "ok", [ln for ln in lines if str(out) not in ln], notes


def symbols(lines):
    """symbol -> body with addresses, encodings, call distances (the literal added to the program
    counter after s_getpc_b64) and the padding behind the function taken out."""
    out, cur, after_pc = {}, None, 0
    for ln in lines:
        m = re.match(r"[0-9a-f]+ <(.+)>:$", ln)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        ins = ln.split("//")[0].strip()
        if after_pc and re.match(r"s_addc?_u32 ", ins):
            ins = ins.rsplit(",", 1)[0] + ", <pc-relative>"
            after_pc -= 1
        else:
            after_pc = 2 if ins.startswith("s_getpc_b64") else 0
        cur.append(ins)
    for body in out.values():   # the padding up to the next function's alignment
        while body and body[-1] in ("s_nop 0", ""):
            body.pop()
    return out


def plain_name(sym):
    """The function's name out of a mangled ``mpcx_kernel::name...`` symbol; other symbols as they are."""
    m = re.match(r"_ZN11mpcx_kernel(\d+)", sym)
    return sym[m.end():m.end() + int(m.group(1))] if m else sym


def compare(job):
    label, src, defines, dirs, work = job
    tag = f"{label:44s} {','.join(defines) or 'main':28s}"
    a, b = (compile_one(src, d, defines, work / f"{abs(hash((label, defines)))}_{i}.hsaco") for i, d in enumerate(dirs))
    if a[0] != b[0]:
        return f"{tag} DIFFERENT: builds {a[0]} against A, {b[0]} against B: {(a if a[0] == 'failed' else b)[1]}"
    if a[0] == "failed":
        same = a[1] == b[1]
        return f"{tag} {'identical' if same else 'DIFFERENT'} (both fail: {'; '.join(a[1])[:160]}{'' if same else ' | ' + '; '.join(b[1])[:160]})"
    if a[1:] == b[1:]:
        return f"{tag} identical ({len(a[1])} lines, {len(symbols(a[1]))} symbols)"
    sa, sb = symbols(a[1]), symbols(b[1])
    diff = [s for s in sorted(set(sa) | set(sb)) if sa.get(s) != sb.get(s)]
    short = [plain_name(s) for s in diff]
    # the metadata lines that changed, as "key: A -> B" (the notes list the same keys in the same order)
    la, lb = a[2].splitlines(), b[2].splitlines()
    meta = [f"{x.strip()} -> {y.split(':', 1)[-1].strip()}" for x, y in zip(la, lb) if x != y] if len(la) == len(lb) else ["layout"]
    return (f"{tag} DIFFERENT: {len(diff)} of {len(sa)} symbols: {', '.join(short) or 'none (addresses or call distances only)'}; "
            f"metadata {'equal' if not meta else 'DIFFERENT: ' + ', '.join(meta)}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("dir_a")
    ap.add_argument("dir_b")
    ap.add_argument("--diag", action="store_true")
    ap.add_argument("--jobs", type=int, default=4)
    args = ap.parse_args()
    dirs = (os.path.abspath(args.dir_a), os.path.abspath(args.dir_b))
    with tempfile.TemporaryDirectory() as tmp:
        work = pathlib.Path(tmp)
        builds = [(p.name, p, d) for p in main_sources() for d in SHIPPED]
        if args.diag:
            builds += diag_builds(work)
        lines = []
        with cf.ThreadPoolExecutor(args.jobs) as ex:
            for line in ex.map(compare, [(*b, dirs, work) for b in builds]):
                lines.append(line)
                print(line, flush=True)
    n = sum("DIFFERENT" in line for line in lines)
    print(f"{len(lines)} builds, {n} different")
    return 1 if n else 0


if __name__ == "__main__":
    sys.exit(main())
