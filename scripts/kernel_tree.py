"""Another IPM kernel tree to compile generated sources against: ``materialise(dst, rev, replace)``
writes the kernel sources (csrc/mpcx_ipm.hip and csrc/ipm/, whichever exist) of the working tree or
of a git revision into ``dst``, with text replacements applied.  Compile with ``-I<dst>`` in front of
``-I<csrc>``: the generated source's ``#include "mpcx_ipm.hip"`` then finds that kernel, while
mpcx_internal.h, mpcx_net_mfma.h and mpcx.h stay the working tree's."""
import pathlib
import shutil
import subprocess

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = "agentlib-mpc_amd/csrc"


def materialise(dst, rev=None, replace=(), unique=False):
    """``rev``: a git revision (None: the working tree; a revision from before the kernel was split
    has the one file only).  ``replace``: (old, new) pairs applied to every file; each ``old`` must
    occur (``unique``: exactly once in all of them).  Returns ``dst``."""
    texts = {}
    if rev is None:
        csrc = ROOT / CSRC
        for p in (csrc / "mpcx_ipm.hip", *sorted((csrc / "ipm").glob("*.h"))):
            texts[p.relative_to(csrc)] = p.read_text()
    else:
        def git(*args):
            return subprocess.run(["git", "-C", str(ROOT), *args], capture_output=True, text=True, check=True).stdout
        for path in git("ls-tree", "-r", "--name-only", rev, "--", f"{CSRC}/mpcx_ipm.hip", f"{CSRC}/ipm").split():
            texts[pathlib.PurePosixPath(path).relative_to(CSRC)] = git("show", f"{rev}:{path}")
    assert "mpcx_ipm.hip" in map(str, texts), f"no kernel source at {rev or 'the working tree'}"
    for old, new in replace:
        found = sum(t.count(old) for t in texts.values())
        assert found == 1 if unique else found >= 1, f"pattern found {found} times: {old!r}"
        texts = {k: t.replace(old, new) for k, t in texts.items()}
    dst = pathlib.Path(dst)
    shutil.rmtree(dst / "ipm", ignore_errors=True)   # of an earlier call with another revision
    for rel, text in texts.items():
        (dst / rel).parent.mkdir(parents=True, exist_ok=True)
        (dst / rel).write_text(text)
    return dst
