"""What kaamer_image_merge and kaamer_makedb_text_range are held to, restated for the tests.

  enumerate_image   E(img) of include/kaamer_hip.h over tableref._Table: the keys whose slot holds a list offset by
                    (offset, key) ascending, each with its ids in stored order, then the keys with an inline id by key
                    ascending.  merge(img_0 ..) is Image.from_pairs over the concatenation of the inputs' enumerations.
  *_entries         the scan loops of pkg/makedb with -offset / -length (inputFASTA.go:64-125, inputEMBL.go:66-119,
                    inputGBK.go:94-118), line for line; their entries go to oracle.makedb_ref's per-entry functions.

Test infrastructure only.  Nothing here calls the library except to obtain the saved image bytes (tableref)."""
import numpy as np

from oracle import makedb_ref as R
from tableref import EMPTY, INLINE, table_of

MAX_INT = 2 ** 63 - 1      # cmd/kaamer-db/main.go:142: the default of -length is uint(MaxInt)
_U64 = 2 ** 64


def enumerate_table(t):
    """E(img) -> (keys uint32, ids uint32)"""
    slots = t.slots.reshape(-1, 2)
    k, v = slots[:, 0], slots[:, 1]
    live = k != EMPTY
    inl = live & ((v & np.uint32(INLINE)) != 0)
    lst = live & ~inl
    lk, lv = k[lst], v[lst]
    order = np.lexsort((lk, lv))                                  # by offset, then by key
    lk, lv = lk[order], lv[order]
    keys, ids = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    if len(lv):
        off, ids = t.ids_csr(lv)
        keys = np.repeat(lk, np.diff(off)).astype(np.uint32)
    ik, iv = k[inl], v[inl] & np.uint32(~INLINE & 0xFFFFFFFF)
    o = np.argsort(ik, kind="stable")
    return np.concatenate([keys, ik[o]]).astype(np.uint32), np.concatenate([ids, iv[o]]).astype(np.uint32)


def enumerate_image(img, tmp_path):
    return enumerate_table(table_of(img, tmp_path, "enum.kgi"))


def enumerate_images(imgs, tmp_path):
    """E(img_0) ++ E(img_1) ++ ... -> (keys, ids)"""
    parts = [enumerate_image(im, tmp_path) for im in imgs]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


# ---- the scan loops with -offset / -length ---------------------------------------------------------------------
def fasta_entries(text, offset=0, length=MAX_INT):
    """inputFASTA.go:64-125 -> [(proteinId, proteinEntry)] in the order they are sent to the jobs channel"""
    jobs = []
    protein_nb = 0                                         # :65
    last_protein = (offset + length) % _U64                # :66 (uint: wraps)
    entry = b""                                            # :93
    for line in R._scan_lines(text):                       # :96
        if len(line) < 1:
            continue                                       # (line[0:1] of an empty line panics: documented divergence)
        if line[0:1] == b">":                              # :98
            protein_nb += 1                                # :99
            if protein_nb >= last_protein:                 # :100
                if entry != b"":                           # :101
                    jobs.append((protein_nb, entry))       # :102
                break                                      # :104 (the entry is not cleared)
            if protein_nb >= offset:                       # :106
                if entry != b"":                           # :107
                    jobs.append((protein_nb, entry))       # :108
                    entry = b""                            # :109
        if protein_nb >= offset:                           # :114
            entry += line + b"\n"                          # :115-116
    if protein_nb >= offset:                               # :120
        if entry != b"":                                   # :121
            jobs.append((protein_nb, entry))               # :122
    return jobs


def flat_entries(text, offset=0, length=MAX_INT):
    """inputEMBL.go:66-119 and inputGBK.go:94-118 (the same loop) -> [(proteinId, proteinEntry)]"""
    jobs = []
    protein_nb = 0                                         # inputEMBL.go:67
    last_protein = (offset + length) % _U64                # :68
    entry = b""                                            # :95
    for line in R._scan_lines(text):                       # :98
        if line == b"//":                                  # :100
            protein_nb += 1                                # :101
            if protein_nb >= last_protein:                 # :102
                jobs.append((protein_nb, entry))           # :103 (empty or not)
                break                                      # :104
            if protein_nb >= offset:                       # :106
                if entry != b"":                           # :107
                    jobs.append((protein_nb, entry))       # :108
                    entry = b""                            # :109
        else:
            if protein_nb >= offset:                       # :113
                entry += line + b"\n"                      # :114-115
    return jobs


def run_fasta_range(text, offset=0, length=MAX_INT):
    """records as makedb_ref.run_fasta gives them.  An entry is one header line (or none) and its sequence lines:
    run_fasta over the entry alone is processProteinInputFASTA (:191-250) on it; the id is the scan loop's."""
    out = []
    for pid, entry in fasta_entries(text, offset, length):
        for _, entry_id, seq, feat in R.run_fasta(entry):
            out.append((pid, entry_id, seq, feat))
    return out


def _run_flat_range(process, text, offset, length):
    """records as makedb_ref.run_embl / run_gbk give them; an entry on which the Go would panic is dropped, as the product does"""
    out = []
    for pid, entry in flat_entries(text, offset, length):
        try:
            r = process(entry)
        except R.RefPanic:
            r = None
        if r is not None:
            entry_id, seq, n, feat = r
            out.append((pid, entry_id, seq[:n], seq, feat))
    return out


def run_embl_range(text, offset=0, length=MAX_INT):
    return _run_flat_range(R.process_embl, text, offset, length)


def run_gbk_range(text, offset=0, length=MAX_INT):
    return _run_flat_range(R.process_gbk, text, offset, length)
