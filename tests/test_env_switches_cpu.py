"""Every PKC_* environment variable the package reads is documented, and nothing else is: the
names the native sources pass to getenv or to the env_* helpers of csrc/pkc_common.h, and the names
pkc/*.py pass to os.environ.get, are exactly the names of INTEGRATION.md's switch table."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-kaldi-cgs_amd")


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _names_read():
    names = set()
    for path in glob.glob(os.path.join(PKG, "csrc", "*")):
        names |= set(re.findall(r'\b(?:getenv|env_str|env_int|env_flag)\(\s*"(PKC_[A-Z0-9_]+)"',
                                _read(path)))
    for path in glob.glob(os.path.join(PKG, "pkc", "*.py")):
        names |= set(re.findall(r'os\.environ\.get\(\s*"(PKC_[A-Z0-9_]+)"', _read(path)))
    return names


def _names_documented():
    rows = re.findall(r"^\| `(PKC_[A-Z0-9_]+)` \|", _read(os.path.join(ROOT, "INTEGRATION.md")),
                      flags=re.M)
    assert len(rows) == len(set(rows)), "a variable is listed twice"
    return set(rows)


def test_switch_table_matches_the_sources():
    read, documented = _names_read(), _names_documented()
    assert len(read) > 20                       # the scan found the readers at all
    assert read - documented == set(), "read but not in INTEGRATION.md's table"
    assert documented - read == set(), "in INTEGRATION.md's table but read nowhere"


def test_native_sources_read_the_environment_through_the_helper_only():
    users = [os.path.basename(p) for p in glob.glob(os.path.join(PKG, "csrc", "*"))
             if re.search(r"\bgetenv\b", _read(p))]
    assert users == ["pkc_common.h"]
