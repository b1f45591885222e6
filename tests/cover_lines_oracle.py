"""Oracle of the cover report's line tables: generateCoverHtml
(syz-manager/cover.go:100-120) and fileSet (cover.go:165-196) restated
literally with Python dicts.  Frames are looked up in a dict from the table
({pc: [(func, file, line), ...]}: what symbolize would return for the PC); the
uncovered set is the C oracle's uncoveredPcsInFuncs
(oracle.pyoracle.cover_uncovered).  Pinned by restatement only: no Go toolchain
is at hand to run the reference's own fileSet."""
import numpy as np

from oracle import pyoracle as O

M64 = (1 << 64) - 1
NO_DATA = "No coverage data available"  # cover.go:93
NO_DEBUG = "does not have debug info"   # cover.go:114


def file_set(covered, uncovered):
    """cover.go:165-196; frames are (func, file, line)."""
    files, funcs = {}, {}
    for func, file, line in covered:
        if file not in files:
            files[file] = {}
        files[file][line] = True
        funcs[func] = True
    for func, file, line in uncovered:
        if not funcs.get(func, False):
            continue
        if file not in files:
            files[file] = {}
        if not files[file].get(line, False):
            files[file][line] = False
    return {f: sorted(lines.items()) for f, lines in files.items()}


def report(cov, base, world, frames=None):
    """cover.go:100-120 up to fileSet.  Returns (fileSet's result, file_seen {file: bits}, covered frames over the
    distinct covered PCs, the covered PCs `frames` does not hold, the uncovered PCs).  A PC that `frames` does not
    hold has no frames."""
    frames = world.frames if frames is None else frames
    cov = np.asarray(cov, dtype=np.uint32)
    if cov.size == 0:
        raise ValueError(NO_DATA)
    pcs = [(((base << 32) + int(c)) - 5) & M64 for c in cov.tolist()]              # cover.go:100-103
    unc = O.cover_uncovered(cov, base, world.sym_start, world.sym_end, world.sites).tolist()  # :104
    covered_frames = [fr for pc in pcs for fr in frames.get(pc, [])]                # :109
    uncovered_frames = [fr for pc in unc for fr in frames.get(pc, [])]              # :117
    seen = {}
    for _, file, _ in covered_frames:
        seen[file] = seen.get(file, 0) | 1
    for _, file, _ in uncovered_frames:
        seen[file] = seen.get(file, 0) | 2
    distinct = sorted(set(pcs))
    ncf = sum(len(frames.get(pc, [])) for pc in distinct)
    missing = [pc for pc in distinct if pc not in frames]
    return file_set(covered_frames, uncovered_frames), seen, ncf, missing, unc


def generate(cov, base, world, frames=None):
    """generateCoverHtml's view: fileSet's result, or the reference's errors."""
    res, _, ncf, _, _ = report(cov, base, world, frames)
    if ncf == 0:
        raise ValueError(NO_DEBUG)                                                  # cover.go:113-115
    return res
