"""CPU: the environment switches the library and the package read are exactly the ones
DESIGN.md's table "Environment switches" lists (no A/B switch comes back unrecorded)."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "waveformer_amd")

_ENV_READ = re.compile(
    r"""os\.(?:environ\.get\(|environ\[|getenv\()\s*["']((?:WF|WAVEFORMER)_\w+)["']"""
    r"""|["']((?:WF|WAVEFORMER)_\w+)["']\s+(?:not\s+)?in\s+os\.environ""")


def _files(root, exts):
    for d, _, names in os.walk(root):
        for n in names:
            if n.endswith(exts):
                yield os.path.join(d, n)


def _read_in_sources():
    names = set()
    for f in _files(os.path.join(PKG, "csrc"), (".hip", ".hpp")):
        names.update(re.findall(r'getenv\(\s*"(\w+)"\s*\)', open(f).read()))
    for f in _files(PKG, (".py",)):
        for m in _ENV_READ.finditer(open(f).read()):
            names.add(m.group(1) or m.group(2))
    return names


def _listed_in_design():
    text = open(os.path.join(REPO, "DESIGN.md")).read()
    m = re.search(r"^#+ [\d.]* *Environment switches\n(.*?)^#+ ", text, re.M | re.S)
    assert m, "DESIGN.md has no 'Environment switches' section"
    return set(re.findall(r"^\| `(\w+)` \|", m.group(1), re.M))


def test_env_switch_inventory_matches_design_table():
    read, listed = _read_in_sources(), _listed_in_design()
    assert read, "found no environment reads: the scan is broken"
    assert read == listed, (f"read but not in DESIGN's table: {sorted(read - listed)}; "
                            f"in the table but not read: {sorted(listed - read)}")
