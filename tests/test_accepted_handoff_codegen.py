"""The written-entry mask of the compact stage image and the hand-off switches (CPU: codegen and
cross-compilation only).

``runtime/codegen.py`` emits ``MPCX_LPW_INIT``: one bit per compact-image entry that some generated
evaluator assigns.  ``local_assemble`` and ``assemble_reg`` (csrc/mpcx_ipm.hip) take 0.0 for every
other entry instead of loading it, so a bit missing from the mask would drop a derivative from the
Newton system: the mask is compared here with the assignments in the generated source itself, for
every structure of ``tests/configs.py``.  The free tail of the image (after the diagonal and the
border) must hold its written entries first, in one run.
"""

import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from agentlib_mpc_amd.runtime import native
from tests import configs

#: the compile-time switches that restore the previous hand-off, part by part
SWITCHES = ["MPCX_GS_HBM", "MPCX_LAM_HBM", "MPCX_HESS_PHASE", "MPCX_LP_ALL"]


def _mask_bits(source):
    words = re.search(r"#define MPCX_LPW_INIT (.*)", source).group(1).split(",")
    bits = set()
    for w, word in enumerate(words):
        v = int(word.strip().removesuffix("ull"), 16)
        bits |= {64 * w + b for b in range(64) if (v >> b) & 1}
    return bits, len(words)


@pytest.mark.parametrize("name", sorted(configs.CASES))
def test_mask_is_the_set_of_assigned_image_entries(name):
    gen = configs.CASES[name]().backend.problem.gen
    ncpt = len(gen.compact)
    # every evaluator body of the source, network variants included, assigns lp[<entry> * S]
    assigned = {int(m.group(1)) for m in re.finditer(r"\blp\[(\d+) \* S\]\s*=", gen.source)}
    assert assigned, "the structure's evaluators write no image entry"
    bits, n_words = _mask_bits(gen.source)
    assert n_words == (ncpt + 63) // 64
    assert bits == assigned == set(gen.lp_written)
    assert max(bits) < ncpt
    # the evaluators never write the border (it comes from the rhs)
    nloc = len(gen.pattern) - 1
    cb, tail0 = nloc + 1, 2 * nloc + 1
    assert not any(cb <= t < tail0 for t in bits)
    # the index tables describe the same entries in the new order
    cij = [int(v) for v in re.search(r"#define MPCX_CIJ_INIT (.*)", gen.source).group(1).split(",")]
    assert cij == [i | (j << 8) for i, j in gen.compact]
    assert gen.compact[:tail0] == [(i, i) for i in range(nloc + 1)] + [(nloc, j) for j in range(nloc)]
    assert len(set(gen.compact)) == ncpt
    # written tail entries first, in one run
    tail_written = sorted(t for t in bits if t >= tail0)
    assert tail_written == list(range(tail0, tail0 + len(tail_written)))


def _compile(source_path, defines):
    cmd = [native._hipcc(), "--cuda-device-only", "-c", f"--offload-arch={native.OFFLOAD_ARCH}", "-O3", "-std=c++17",
           f"-I{native.INCLUDE}", f"-I{native.CSRC}", *[f"-D{d}" for d in defines], str(source_path), "-o", "/dev/null"]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_every_switch_compiles_alone_and_together(tmp_path):
    gen = configs.one_room().backend.problem.gen
    src = tmp_path / "one_room.hip"
    src.write_text(gen.source)
    combos = [[s] for s in SWITCHES] + [SWITCHES]
    with ThreadPoolExecutor(len(combos)) as ex:
        for defines, res in zip(combos, ex.map(lambda d: _compile(src, d), combos)):
            assert res.returncode == 0, (defines, res.stderr[-2000:])
