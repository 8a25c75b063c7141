"""The compile-time switches of the device sources are a closed list: every
GCMX_* macro a preprocessor conditional of gcm_amd/csrc tests is named here, so
a new one has to be added on purpose (the settled tuning macros were frozen at
their shipped values, docs/HISTORY.md "Tuning macros retired")."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gcm_amd", "csrc")

KNOBS = {
    # kernels_xyz.hip / kernels_ortho.hip / iso.hpp: the two floating-point builds
    "GCMX_FMA",
    # kernels_xyz.hip: per-block timing build (scripts/r6/diag_blk.py); selects no code path
    "GCMX_TX2_BLKT",
    # kernels_fast.hip
    "GCMX_MARCH_MINWAVES",
    "GCMX_MARCH_CHUNK",
    # kernels_2d.hip
    "GCMX_2D_PF",
    # simplex.hip
    "GCMX_SX_L8_BLOCK",
    "GCMX_SX_GPOLL_SLEEP",
    "GCMX_SX_L8_STAGE",
    "GCMX_SX_DIAG_NOCORR",
    "GCMX_SX_DIAG_TWICE",
    "GCMX_SX_DIAG_ASINNER",
}


def test_the_compile_time_switches_are_the_listed_ones():
    found = {}
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")))
    assert files
    for path in files:
        with open(path) as f:
            for line in f:
                if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", line):
                    for name in re.findall(r"GCMX_[A-Z0-9_]+", line):
                        found.setdefault(name, os.path.basename(path))
    assert set(found) == KNOBS, (
        f"not listed: {sorted((n, found[n]) for n in set(found) - KNOBS)}, "
        f"listed but gone: {sorted(KNOBS - set(found))}")
