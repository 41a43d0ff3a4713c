"""The forms kaamer_amd/api.py serves from one body each: the full hit lists (flat and struct, search and submit, with and
without bitmaps) and the reported hits (flat, struct, with bitmaps, with alignments; search and submit) on an Index and
on a ShardedIndex, and the stream-open forms on the three handle kinds.  Every form returns what its neighbour returns on
the same input -- the neighbours are the forms the other tests hold against the oracle.  Other tests reach all of these
but Index.search(flat=False, want_positions=True); here each stands next to its neighbour on the smallest input that
takes the path: 40 proteins, a few queries (one empty), two shards, everything on device 0."""
import pytest

from test_sharded_top_align import ALN, _same_top
from test_top_align import _fasta

K = 5
FORMS = {"flat": {}, "struct": dict(flat=False), "pos": dict(want_positions=True), "aln": dict(align=ALN),
         "pos+aln": dict(want_positions=True, align=ALN)}


@pytest.fixture(scope="module")
def small(klib, gpu_device):
    from kaamer_amd import abi, api, workload
    db = workload.make_db(40, seed=71)
    prot = api.Proteins.from_fasta(_fasta(workload.unpack(db)).encode())
    handles = dict(index=api.Index.from_image(prot.image(device=gpu_device), gpu_device),
                   sharded=api.ShardedIndex.from_images([prot.image(shard=r, n_shards=2, device=gpu_device) for r in range(2)],
                                                        [gpu_device] * 2),
                   replicas=api.Replicas.from_image(prot.image(device=gpu_device), [gpu_device, gpu_device]))
    for h in handles.values():
        h.attach_proteins(prot)
    queries = workload.unpack(workload.make_protein_queries(db, 3, seed=72))
    batches = {"protein": (api.pack_sequences(queries[:2] + [b""] + queries[2:]), abi.PROTEIN),
               "reads": (workload.make_reads(db, 4, seed=73), abi.READS)}
    refs = {}

    def ref(kind, form):
        """Index.search_top of the batch in that form, computed once"""
        if (kind, form) not in refs:
            packed, seq_type = batches[kind]
            refs[kind, form] = handles["index"].search_top(packed=packed, seq_type=seq_type, max_results=K, **FORMS[form])
        return refs[kind, form]
    yield dict(handles=handles, batches=batches, ref=ref)
    for h in handles.values():
        h.close()


def _same_full(got, ref, positions):
    assert got.n_queries == ref.n_queries and got.meta.tolist() == ref.meta.tolist()
    assert got.hit_cnt.tolist() == ref.hit_cnt.tolist() and bytes(got.orf_aa) == bytes(ref.orf_aa)
    assert (got.pos_bits is not None) == (ref.pos_bits is not None) == positions
    for q in range(ref.n_queries):
        assert got.hits(q) == ref.hits(q) and got.first_pos(q) == ref.first_pos(q), q
        if positions:
            a, b = got.positions(q), ref.positions(q)
            assert a.keys() == b.keys() and all(a[p].tolist() == b[p].tolist() for p in b), q


@pytest.mark.gpu
@pytest.mark.parametrize("positions", (False, True), ids=("plain", "pos"))
@pytest.mark.parametrize("handle", ("index", "sharded"))
def test_full_list_forms_agree(small, handle, positions):
    h = small["handles"][handle]
    for kind, (packed, seq_type) in small["batches"].items():
        ref = small["handles"]["index"].search(packed=packed, seq_type=seq_type, want_positions=positions)
        assert sum(ref.hit_cnt.tolist()) > 0
        _same_full(h.search(packed=packed, seq_type=seq_type, want_positions=positions, flat=False), ref, positions)
        _same_full(h.submit(packed=packed, seq_type=seq_type, want_positions=positions).wait(), ref, positions)
        if handle == "sharded":
            _same_full(h.search(packed=packed, seq_type=seq_type, want_positions=positions), ref, positions)


@pytest.mark.gpu
@pytest.mark.parametrize("form", tuple(FORMS))
@pytest.mark.parametrize("handle", ("index", "sharded"))
def test_top_forms_agree(small, handle, form):
    h = small["handles"][handle]
    for kind, (packed, seq_type) in small["batches"].items():
        ref = small["ref"](kind, form)
        assert ref.n_reported > 0 and (ref.pos_bits is not None) == ("pos" in form) and (ref.alignments is not None) == ("aln" in form)
        if form in ("flat", "struct"):               # the struct form returns what the flat form returns
            _same_top(ref, small["ref"](kind, "flat"))
        if handle == "sharded":
            _same_top(h.search_top(packed=packed, seq_type=seq_type, max_results=K, **FORMS[form]), ref)
        if form == "struct" and handle == "sharded":   # ShardedIndex.submit_top has no struct form
            continue
        _same_top(h.submit_top(packed=packed, seq_type=seq_type, max_results=K, **FORMS[form]).wait(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ("flat", "pos", "aln", "pos+aln"))
@pytest.mark.parametrize("handle", ("index", "replicas", "sharded"))
def test_stream_open_forms_agree(small, handle, form):
    kw = {k: v for k, v in FORMS[form].items()}
    for kind, (packed, seq_type) in small["batches"].items():
        st = small["handles"][handle].stream(seq_type, max_results=K, **kw)
        assert st.push(*packed) and st.pending == 1
        _same_top(st.pop(), small["ref"](kind, form))
        assert st.pending == 0
        st.close()
        st.close()                                    # idempotent
