"""k_bgzf.hip for gfx950: every kernel without VGPR spills and without scratch (tools/isa_stats.sh)."""
import os
import re
import subprocess

from util import ROOT


def test_bgzf_kernels_no_spills_no_scratch():
    p = subprocess.run(["bash", os.path.join(ROOT, "tools", "isa_stats.sh"), "k_bgzf"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    rows = [l for l in p.stdout.splitlines() if "VGPR spills" in l]
    names = [l.split()[0] for l in rows]
    assert any("k_bgzf_blocks" in n for n in names) and any("k_bgzf_scan" in n for n in names) and any("k_bgzf_compact" in n for n in names), p.stdout
    for l in rows:
        m = re.search(r"VGPR spills\s+(\d+) \(scratch\s+(\d+) B\)", l)
        assert m and m.group(1) == "0" and m.group(2) == "0", l
