"""Generates the fixture that pins the library's thirteen genetic codes to the reference's own text.

Run with a checkout of the reference, read as TEXT only (the reference is Go and
is not executed):

    python tests/golden/make_gcode_fixtures.py <reference checkout>

Output (data only, no reference source text):
  gcodes.json   "<code>" -> codon -> [AA, Start, Stop] for every key of search.GCodes
                (1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14, 15), parsed from the map literals
                gcode_N of pkg/search/gcode.go:103-972

The reference cites an older listing than today's NCBI pages and its start sets are narrower:
the library must equal THESE maps.
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CODES = (1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14, 15)


def gcodes(ref):
    src = open(os.path.join(ref, "pkg/search/gcode.go")).read()
    listed = re.search(r"var GCodes = map\[int\]map\[string\]AminoAcid\{(.*?)\}", src, re.S).group(1)
    keys = tuple(int(k) for k, n in re.findall(r"(\d+):\s*gcode_(\d+)", listed) if k == n)
    assert keys == CODES, keys
    out = {}
    for code in CODES:
        m = re.search(r"var gcode_%d = map\[string\]AminoAcid\{(.*?)\n\}" % code, src, re.S)
        rows = re.findall(r'"([a-z]{3})":\s*AminoAcid\{AA:\s*"(.)",\s*Start:\s*(true|false),\s*Stop:\s*(true|false)\}', m.group(1))
        table = {codon: [aa, start == "true", stop == "true"] for codon, aa, start, stop in rows}
        assert len(rows) == 64 and len(table) == 64, (code, len(rows), len(table))      # 64 distinct codons
        assert all(len(c) == 3 and set(c) <= set("tcag") for c in table), code
        for codon, (aa, start, stop) in table.items():
            assert stop == (aa == "*"), (code, codon)                                    # Stop <=> AA '*'
            assert not (start and stop), (code, codon)
        out[str(code)] = table
    bacteria = json.load(open(os.path.join(HERE, "gcode_bacteria.json")))
    assert out["11"] == bacteria, "gcode_11 differs from gcodeBacteria"
    return out


if __name__ == "__main__":
    tables = gcodes(sys.argv[1])
    with open(os.path.join(HERE, "gcodes.json"), "w") as f:
        json.dump(tables, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote gcodes.json: %d codes x 64 codons" % len(tables))
