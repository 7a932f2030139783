"""The environment variables the library reads and the knob table of INTEGRATION.md section 4 name the same set, and one source
file alone reads the environment (the option table of csrc/hpe_plan.hip, resolved once per context)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "human-pose-estimation_amd", "csrc")


def _getenv_files():
    out = []
    for f in sorted(os.listdir(CSRC)):
        text = open(os.path.join(CSRC, f)).read()
        if re.search(r"\bgetenv\s*\(", text):
            out.append(f)
    return out


def test_one_file_reads_the_environment():
    assert _getenv_files() == ["hpe_plan.hip"]


def test_no_static_caches_an_environment_value():
    # the idiom the launchers used: `static const int v = [] { ... getenv ... }();`
    text = open(os.path.join(CSRC, "hpe_plan.hip")).read()
    assert not re.search(r"static[^;{]*=\s*\[[^\]]*\]\s*(\([^)]*\))?\s*\{[^}]*getenv", text)


def test_knob_table_matches_the_code():
    text = open(os.path.join(CSRC, "hpe_plan.hip")).read()
    # every getenv call goes through the option table: its argument is the env column of a row, never a literal elsewhere
    assert re.findall(r"\bgetenv\s*\(([^)]*)\)", text) == ["o.env"]
    in_code = set(re.findall(r'"(HPE_[A-Z0-9_]+)"', text))
    assert len(in_code) >= 20
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    in_doc = set()
    for line in doc.splitlines():
        m = re.match(r"\|\s*`(HPE_[A-Z0-9_]+)`\s*\|", line)
        if m:
            in_doc.add(m.group(1))
    assert in_code - in_doc == set(), "read by the library, missing in the INTEGRATION.md table"
    assert in_doc - in_code == set(), "in the INTEGRATION.md table, not read by the library"
