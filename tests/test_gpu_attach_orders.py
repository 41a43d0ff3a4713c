"""The three attaches of an index (attach_proteins, attach_subject_text, attach_subject_json) in every order, and each of them
replaced afterwards: the id -> entry map is built by one attach and borrowed by the others, and handed on when its builder
goes.  After every step one small text call of every format whose attaches are present equals the host formatter on the
table that format's attach holds; the info numbers say who built a map and who borrowed one."""
import itertools

import pytest

import tsvcases
import writercases as W
from kaamer_amd import api

pytestmark = pytest.mark.gpu

ATTACH = dict(proteins="attach_proteins", text="attach_subject_text", json="attach_subject_json")


@pytest.fixture(scope="module")
def setup(klib, gpu_device):
    full = tsvcases.standard_table()
    short = W.short_table(full)
    text, seqs = W.queries()
    img = full.image()
    own = {}                       # table_bytes of an attach that builds its own map, per attach and table
    for kind in ATTACH:
        for name, table in (("full", full), ("short", short)):
            ix = api.Index.from_image(img, gpu_device)
            getattr(ix, ATTACH[kind])(table)
            own[kind, name] = _bytes(ix, kind)
            ix.close()
    yield dict(img=img, tables=dict(full=full, short=short), text=text, seqs=seqs, own=own, device=gpu_device)


def _bytes(ix, kind):
    return dict(proteins=ix.align_info, text=ix.subject_text_info, json=ix.subject_json_info)[kind]()["table_bytes"]


class Tracked:
    """an index and the table each of its attaches holds"""

    def __init__(self, s):
        self.s, self.ix, self.held = s, api.Index.from_image(s["img"], s["device"]), {}

    def attach(self, kind, name):
        s, table = self.s, self.s["tables"][name]
        if kind == "text":         # text borrows the alignment table's map; JSON the text's, else the alignment table's
            borrows = self.held.get("proteins") == name
        elif kind == "json":
            borrows = self.held.get("text") == name or self.held.get("proteins") == name
        else:
            borrows = False        # attach_proteins always builds
        getattr(self.ix, ATTACH[kind])(table)
        self.held[kind] = name
        max_id = len(table) - 1
        assert _bytes(self.ix, kind) == s["own"][kind, name] - (4 * (max_id + 2) if borrows else 0), (kind, name, self.held)
        self.check_calls()

    def check_calls(self):
        s, held = self.s, self.held
        if "text" in held:
            W.check(W.call(self.ix, "tsv", s["text"]), "tsv", s["text"], s["seqs"], s["tables"][held["text"]])
        if "text" in held and "proteins" in held:
            got = W.check(W.call(self.ix, "align+tsv", s["text"]), "align+tsv", s["text"], s["seqs"], s["tables"][held["text"]])
            missing = [a["status"] == 4 for a in got.alignments]
            assert any(missing) == (held["proteins"] == "short") and not all(missing)
        if "json" in held:
            W.check(W.call(self.ix, "json", s["text"]), "json", s["text"], s["seqs"], s["tables"][held["json"]])


@pytest.mark.parametrize("order", list(itertools.permutations(ATTACH)), ids="-".join)
def test_attach_order_then_replace_each(setup, order):
    t = Tracked(setup)
    try:
        for kind in order:
            t.attach(kind, "full")
        for kind in ATTACH:
            t.attach(kind, "full")     # the same table again: the old attach goes first, its map moves to a borrower
            t.attach(kind, "short")    # a table that lacks a reported entry: the missing-entry rule shows in that format
            t.attach(kind, "full")
    finally:
        t.ix.close()


def test_the_missing_entry_shows(setup):
    """the short table under each writer changes that writer's bytes and no other's"""
    s = setup
    t = Tracked(s)
    try:
        for kind in ATTACH:
            t.attach(kind, "full")
        base = {f: W.call(t.ix, f, s["text"]) for f in ("tsv", "align+tsv", "json")}
        for kind, changed in (("text", {"tsv", "align+tsv"}), ("json", {"json"}), ("proteins", {"align+tsv"})):
            t.attach(kind, "short")
            for f, b in base.items():
                got = W.call(t.ix, f, s["text"])
                same = (got.tsv, got.json) == (b.tsv, b.json)
                assert same == (f not in changed), (kind, f)
            t.attach(kind, "full")
    finally:
        t.ix.close()
