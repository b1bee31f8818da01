"""CPU checks of the library's environment switches, read from the sources as text: csrc/knobs.h is the only file of csrc/ that reads
the environment, and its comment table lists every DINOX_* name the kernel sources mention."""
import glob
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "dino-x_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "dinox.h")
TOKEN = re.compile(r"DINOX_[A-Z0-9_]+")


def sources():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert len(files) >= 30 and os.path.join(CSRC, "knobs.h") in files
    return files


def test_getenv_only_in_knobs_h():
    offenders = [os.path.basename(f) for f in sorted(glob.glob(os.path.join(CSRC, "*"))) if os.path.isfile(f)
                 and os.path.basename(f) != "knobs.h" and "getenv" in open(f, errors="replace").read()]
    assert offenders == [], f"getenv outside csrc/knobs.h: {offenders}"
    assert "getenv" in open(os.path.join(CSRC, "knobs.h")).read()


def test_every_knob_is_listed_in_knobs_h():
    abi = set(TOKEN.findall(open(HEADER).read()))                 # DINOX_EPI_*, error codes, DINOX_F32 / DINOX_BF16, ABI version
    assert {"DINOX_EPI_GELU", "DINOX_EUNSUPPORTED", "DINOX_F32", "DINOX_BF16"} <= abi
    table = set()
    for line in open(os.path.join(CSRC, "knobs.h")):
        m = re.match(r"//\s{3}(DINOX_[A-Z0-9_]+)\s{2,}\S", line)     # a table row: the name, then its description
        if m:
            table.add(m.group(1))
    assert len(table) >= 19 and not (table & abi)
    missing = {}
    for f in sources():
        for tok in set(TOKEN.findall(open(f).read())) - abi - table:
            missing.setdefault(tok, []).append(os.path.basename(f))
    assert missing == {}, f"DINOX_* names used in csrc/ but not in the knobs.h table: {missing}"
    # and the table names nothing that no source reads (rows of the 'not read here' section are named in comments or #ifdef)
    used = set()
    for f in sources():
        if os.path.basename(f) != "knobs.h":
            used |= set(TOKEN.findall(open(f).read()))
    assert table <= used, f"knobs.h lists names that csrc/ no longer mentions: {sorted(table - used)}"
