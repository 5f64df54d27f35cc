"""The column order of the ingest's pointer table is stated once, as ``TDT_COL_*`` in include/tiddit_hip.h: its Python face
(``bamio._FIELDS`` + ``raw``) and the test suite's own restatement (``ingest_cases.COLUMNS``) are that order."""
import os
import re

import ingest_cases

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _enum():
    hdr = open(os.path.join(REPO, "include", "tiddit_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    body = re.search(r"enum\s*\{\s*(TDT_COL_TID\b[^}]*)\}", hdr).group(1)
    names, value = [], 0
    for item in (x.strip() for x in body.split(",")):
        m = re.fullmatch(r"(\w+)(?:\s*=\s*(\d+))?", item)
        value = int(m.group(2)) if m.group(2) else value
        names.append((m.group(1), value))
        value += 1
    return names


def test_the_enum_is_the_order_of_the_python_table_and_of_the_ingest_cases():
    from tiddit_amd import bamio
    names = _enum()
    assert [v for _, v in names] == list(range(len(names)))
    assert names[-1] == ("TDT_NCOL", 14)
    cols = [n[len("TDT_COL_"):].lower() for n, _ in names[:-1]]
    assert all(n.startswith("TDT_COL_") for n, _ in names[:-1])
    assert cols == [name for name, _ in bamio._FIELDS] + ["raw"]
    assert cols == list(ingest_cases.COLUMNS) + ["raw"]
