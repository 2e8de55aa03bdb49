"""The code-format table of million_amd/ops.py, without a GPU: ops.code_format returns the instance each public op
documents for what it is handed, refuses the mismatches the ops refuse, with their messages, and every C entry the table names is
one that _lib.SYMBOLS prototypes."""
import dataclasses

import pytest
import torch

from million_amd import _lib as L
from million_amd import ops

U8, U16 = torch.uint8, torch.uint16


def test_the_three_formats():
    assert ops.CODE_FORMATS == (ops.FMT_U8, ops.FMT_U16, ops.FMT_PACKED) and len({f.name for f in ops.CODE_FORMATS}) == 3
    # (dtype of the stores, a row-major form, code_bytes of the gather's descriptor, the prepared blob)
    assert [(f.dtype, f.rowmajor, f.code_bytes, f.prepared) for f in ops.CODE_FORMATS] == [(U8, True, 1, True), (U16, True, 2, False), (U8, False, 2, False)]
    assert ops.FMT_U16.centroids == ops.FMT_PACKED.centroids == ops.WIDE_CENTROIDS == (512, 1024, 2048, 4096)
    assert all(C in ops.FMT_U8.centroids for C in (1, 2, 16, 128, 256)) and 0 not in ops.FMT_U8.centroids and 257 not in ops.FMT_U8.centroids
    assert ops.FMT_U8.page_shapes(64, 32, 256) == ops.FMT_U16.page_shapes(64, 32, 4096) == ((64, 32), (32, 64))
    assert ops.FMT_PACKED.page_shapes(64, 32, 4096) == ((ops.packed_page_bytes(64, 32, 4096),),) * 2 == ((3072,), (3072,))
    with pytest.raises(Exception):      # immutable
        ops.FMT_U8.code_bytes = 2


@pytest.mark.parametrize("dtype, C, packed, want", [
    (U8, 256, False, "FMT_U8"), (U8, 16, False, "FMT_U8"), (U8, 1, False, "FMT_U8"),                     # pq_chunk_attn, pq_gather_rows: any C <= 256
    (U16, 512, False, "FMT_U16"), (U16, 1024, False, "FMT_U16"), (U16, 2048, False, "FMT_U16"), (U16, 4096, False, "FMT_U16"),
    (U8, 512, True, "FMT_PACKED"), (U8, 1024, True, "FMT_PACKED"), (U8, 2048, True, "FMT_PACKED"), (U8, 4096, True, "FMT_PACKED"),
    (U8, None, False, "FMT_U8"), (U16, None, False, "FMT_U16"), (U8, None, True, "FMT_PACKED"),          # pq_chunk_attn_blocks: the dtype and the flag
])
def test_code_format_picks(dtype, C, packed, want):
    assert ops.code_format("op", dtype, C, packed) is getattr(ops, want)
    if not packed:
        assert ops.code_format("op", dtype, C) is getattr(ops, want)      # the flag defaults to off: a uint8 pool means 8-bit codes


@pytest.mark.parametrize("dtype, C, packed, msg", [
    (U8, 1024, False, r"op: C=1024 does not go with torch.uint8 codes \(uint8: C <= 256; uint16: C in \(512, 1024, 2048, 4096\)\)"),
    (U8, 256, True, r"packed codes: C=256 \(packed pages hold codes of \(512, 1024, 2048, 4096\) centroids; C <= 256 is a uint8 already\)"),
    (U16, 768, False, r"op: C=768 does not go with torch.uint16 codes"),
    (U16, 256, False, "C=256 does not go with torch.uint16"), (U16, 8192, False, "C=8192 does not go with"), (U8, 768, True, "packed codes: C=768"),
    (torch.int16, 1024, False, "op: codes must be uint8 or uint16, both sides alike"), (torch.float16, None, False, "codes must be uint8 or uint16"),
])
def test_code_format_refuses(dtype, C, packed, msg):
    with pytest.raises(RuntimeError, match=msg):
        ops.code_format("op", dtype, C, packed)


def test_the_ops_refuse_with_the_same_words(monkeypatch):
    """pq_gather_rows is the op that picks the format from what it is handed: its refusals are code_format's."""
    monkeypatch.setattr(ops, "_need_cuda", lambda *a: None)
    monkeypatch.setattr(ops.L, "load", lambda: pytest.fail("the library was entered"))
    h = torch.float16
    ids = torch.zeros(1, 2, 2, dtype=torch.int32)
    out = torch.zeros(1, 2, 100, 128, dtype=h)
    gather = lambda pool, C, **kw: ops.pq_gather_rows(pool, pool, torch.zeros(64, C, 2, dtype=h), torch.zeros(64, C, 2, dtype=h), out, out.clone(),
                                                     t0=0, t1=90, k_page_ids=ids, v_page_ids=ids, page_size=64, **kw)
    with pytest.raises(RuntimeError, match="pq_gather_rows: C=1024 does not go with torch.uint8 codes"):
        gather(torch.zeros(4, 64 * 64 * 10 // 8, dtype=U8), 1024)
    with pytest.raises(RuntimeError, match="packed codes: C=256"):
        gather(torch.zeros(4, 64 * 64, dtype=U8), 256, packed=True)
    with pytest.raises(RuntimeError, match="pq_gather_rows: C=768 does not go with torch.uint16 codes"):
        gather(torch.zeros(4, 64, 64, dtype=U16), 768)


def test_every_entry_of_the_table_is_prototyped():
    for f in ops.CODE_FORMATS:
        for field in ("encode", "decode_attn", "decode_ws", "chunk_attn", "chunk_attn_lse", "chunk_ws", "gather"):
            assert getattr(f, field) in L.SYMBOLS, (f.name, field)
        for field in ("op_decode_attn", "op_chunk_attn"):
            assert callable(getattr(ops, getattr(f, field))), (f.name, field)
        for job in ("encode_pages", "decode_workspace", "decode_pages", "chunk_op"):      # what a paged cache asks of its format
            assert callable(getattr(f, job)), (f.name, job)
    assert not [x.name for x in dataclasses.fields(ops.CodeFormat) if x.name.startswith("op_") and x.name not in ("op_decode_attn", "op_chunk_attn")]
    # one entry per format where the formats differ, one shared entry where they do not
    assert len({f.decode_attn for f in ops.CODE_FORMATS}) == len({f.chunk_attn for f in ops.CODE_FORMATS}) == 3
    assert ops.FMT_U8.gather == ops.FMT_U16.gather != ops.FMT_PACKED.gather and ops.FMT_U8.encode == ops.FMT_U16.encode != ops.FMT_PACKED.encode
    assert ops.FMT_U8.chunk_attn != ops.FMT_U8.chunk_attn_lse and all(f.chunk_attn == f.chunk_attn_lse for f in (ops.FMT_U16, ops.FMT_PACKED))


def test_the_jobs_hand_each_op_its_own_keywords(monkeypatch):
    """One call shape per job from the cache's side; the format adds what its op takes, and finds the op when it is called."""
    log = []
    for name in ("pq_encode_into", "pq_encode_into_packed", "pq_decode_attn", "pq_decode_attn_wide", "pq_decode_attn_packed", "pq_chunk_attn",
                 "pq_chunk_attn_wide", "pq_chunk_attn_packed", "pq_chunk_attn_blocks", "decode_workspace_bytes", "decode_wide_workspace_bytes"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: log.append((_n, a, k)))
    cents, prep, res = ("kc", "vc"), ("kp", "vp"), torch.zeros(1, 2, 8, 128)
    for f, enc, dec, chunk in ((ops.FMT_U8, "pq_encode_into", "pq_decode_attn", "pq_chunk_attn"), (ops.FMT_U16, "pq_encode_into", "pq_decode_attn_wide", "pq_chunk_attn_wide"),
                               (ops.FMT_PACKED, "pq_encode_into_packed", "pq_decode_attn_packed", "pq_chunk_attn_packed")):
        del log[:]
        f.encode_pages("X", "cent", "img", "pool", layout=1, n=3)
        assert log[-1] == (enc, ("X", "cent", "pool"), dict(layout=1, n=3, **({"prepared": "img"} if f.rowmajor else {})))
        f.decode_workspace("q", res, M=64, C=256, page_size=32)
        assert log[-1] == (("decode_workspace_bytes", ("q", res), dict(nh_k=2, M=64, C=256)) if f.prepared else
                           ("decode_wide_workspace_bytes", ("q", res), dict(M=64, C=256, page_size=32)))
        f.decode_pages("q", "kpool", "vpool", cents, prep, "kres", "vres", 5, M=64, C=256, page_ids="ids", n_tokens=7, k_new="row")
        said = dict(M=64, C=256, k_page_ids="ids", v_page_ids="ids") if f.prepared else dict(page_ids="ids")
        assert log[-1] == (dec, ("q", "kpool", "vpool", *(prep if f.prepared else cents), "kres", "vres", 5), dict(n_tokens=7, k_new="row", **said))
        for route, op, extra in ((None, chunk, {}), ("chunk", chunk, {}), ("blocks", "pq_chunk_attn_blocks", {} if f.rowmajor else {"packed": True})):
            f.chunk_op("who", route)("q", "k", "v", "kpool", "vpool", cents, prep, "kres", "vres", 5, M=64, n_tokens=7)
            assert log[-1] == (op, ("q", "k", "v", "kpool", "vpool", *(prep if f.prepared else cents), "kres", "vres", 5), dict(M=64, n_tokens=7, **extra))
        with pytest.raises(ValueError, match=r"who: route='rows' \(None, 'chunk' or 'blocks'\)"):
            f.chunk_op("who", "rows")
