"""The host front the two ragged-store entries of the C ABI share (csrc/store_ragged.hip: store_ragged_front), without a GPU:
million_pq_store_ragged and million_pq_store_ragged_wide refuse the same bad calls on the same rungs, in the same order, each
with its own return code and words.  Every call here is refused (or is the empty call) before a launch: the addresses are made up."""
import ctypes

import pytest

from tests.test_attn_wide_host import A, ERR_ALIGN, ERR_ARG, ERR_SHAPE, lib      # noqa: F401 (lib: the fixture)

# (entry, its name in the messages, C of a good call, a C its geometry refuses with a fragment of those words,
#  the fragments of its two own messages: null codebook, 16-byte alignment)
ENTRIES = [
    ("million_pq_store_ragged", b"store_ragged: ", 256, (512, b"M 16 / 32 / 64, C 1 .. 256: uint8 codes"),
     b"null prepared codebook (million_prepare_cents: the call needs both)", b"rows, windows, prepared codebooks and pools must be 16-byte aligned"),
    ("million_pq_store_ragged_wide", b"store_ragged_wide: ", 1024, (256, b"C 512 / 1024 / 2048 / 4096; packed pages: M a multiple of 4"),
     b"null codebook (the plain (M, C, d_m) fp16 tensors: the call needs both)", b"rows, windows, codebooks and pools must be 16-byte aligned"),
]
# the pointer arguments in call order; `packed` and the stream follow them
PTRS = ["k_new", "v_new", "k_resid", "v_resid", "k_cents", "v_cents", "k_pool", "v_pool", "page_ids", "dev_lengths", "dev_n"]


def _good(L, C):
    d = L.StoreRaggedDesc()
    d.struct_size = ctypes.sizeof(L.StoreRaggedDesc)
    d.bs, d.nh_k, d.d, d.M, d.C, d.n_bound = 3, 2, 128, 64, C, 40
    d.kn_stride_b, d.kn_stride_h, d.kn_stride_n = 2 * 40 * 128, 40 * 128, 128
    d.vn_stride_b, d.vn_stride_h, d.vn_stride_n = 2 * 40 * 128, 40 * 128, 128
    d.resid_cap, d.page_size, d.n_pages_cap = 128, 64, 70
    d.resid_stride_b, d.resid_stride_h = 2 * 128 * 128, 128 * 128
    return d, {name: A + 0x10000 * i for i, name in enumerate(PTRS)}


def _set(**fields):
    def f(d, p, entry):
        for k, v in fields.items():
            setattr(d, k, v)
    return f


def _ptr(name, value):
    def f(d, p, entry):
        p[name] = None if value is None else p[name] + value
    return f


def _rungs(entry):
    """The refusal ladder, top down: (what, the change that makes a good call bad on this rung, code, fragment of the message)."""
    _, _, _, (bad_C, geometry_words), null_cents_words, align16_words = entry
    return [
        ("struct_size", _set(struct_size=8), ERR_ARG, b"bad desc / struct_size"),
        ("bs", _set(bs=0), ERR_SHAPE, b"bs=0 nh_k="),
        ("nh_k", _set(nh_k=0), ERR_SHAPE, b"nh_k=0 n_bound="),
        ("n_bound", _set(n_bound=-1), ERR_SHAPE, b"n_bound=-1"),
        ("geometry", _set(C=bad_C), ERR_SHAPE, geometry_words),
        ("page_size", _set(page_size=48), ERR_SHAPE, b"page_size=48 (32, 64 or 128)"),
        ("n_pages_cap", _set(n_pages_cap=0), ERR_SHAPE, b"n_pages_cap=0 (page table of 0 entries)"),
        ("grid", _set(bs=4096, nh_k=8), ERR_SHAPE, b"bs * nh_k = 32768 exceeds the grid (32767)"),
        ("resid_cap", _set(resid_cap=-1), ERR_ARG, b"resid_cap=-1"),
        ("dev_n", _ptr("dev_n", None), ERR_ARG, b"null dev_n (the row count of every request is read on the device)"),
        ("dev_lengths", _ptr("dev_lengths", None), ERR_ARG, b"null dev_lengths"),
        ("window", _ptr("v_resid", None), ERR_ARG, b"null window with resid_cap=128"),
        ("codebook", _ptr("v_cents", None), ERR_ARG, null_cents_words),
        ("rows / pools / ids", _ptr("k_pool", None), ERR_ARG, b"null new rows / pools / page_ids"),
        ("16 bytes", _ptr("k_cents", 8), ERR_ALIGN, align16_words),
        ("4 bytes", _ptr("page_ids", 2), ERR_ALIGN, b"page_ids / dev_lengths / dev_n must be 4-byte aligned"),
        ("strides", _set(vn_stride_h=40 * 128 + 4), ERR_ALIGN, b"fp16 strides must be multiples of 8 elements (16-byte rows)"),
    ]


def _call(lib, entry, d, p, packed=0):
    args = [p[name] for name in PTRS] + ([packed] if entry[0].endswith("_wide") else [])
    return getattr(lib, entry[0])(ctypes.byref(d), *args, None)


N_RUNGS = 17


@pytest.mark.parametrize("entry", ENTRIES, ids=[e[0] for e in ENTRIES])
@pytest.mark.parametrize("i", range(N_RUNGS))
@pytest.mark.parametrize("later_too", [False, True], ids=["alone", "with every later rung's fault"])
def test_bad_calls_are_refused_rung_by_rung(lib, entry, i, later_too):
    """One table of bad calls against both entries.  alone: the call is bad on rung i only.  With every later rung's fault as well
    (applied first, so rung i's change stands where two touch one field) the answer is still rung i's: the order of the ladder."""
    from million_amd import _lib as L
    rungs = _rungs(entry)
    assert len(rungs) == N_RUNGS
    what, _, code, words = rungs[i]
    d, p = _good(L, entry[2])
    for _, change, _, _ in reversed(rungs[i:] if later_too else rungs[i:i + 1]):
        change(d, p, entry)
    assert _call(lib, entry, d, p) == code, (what, lib.million_last_error())
    msg = lib.million_last_error()
    assert msg.startswith(entry[1]) and words in msg, (what, msg)


def test_packed_pages_meet_the_same_geometry_rung(lib):
    """packed = 1 on the wide entry: the geometry rung answers with the same words."""
    from million_amd import _lib as L
    entry = ENTRIES[1]
    d, p = _good(L, entry[3][0])
    assert _call(lib, entry, d, p, packed=1) == ERR_SHAPE and entry[3][1] in lib.million_last_error()


@pytest.mark.parametrize("entry", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_no_row_bound_is_ok_whatever_the_pointers(lib, entry):
    """n_bound == 0: no request can have a row - MILLION_OK before any pointer is looked at; the checks of the shape in front of it
    still refuse."""
    from million_amd import _lib as L
    d, p = _good(L, entry[2])
    d.n_bound = 0
    assert _call(lib, entry, d, dict.fromkeys(PTRS)) == 0
    assert _call(lib, entry, d, {name: 1 for name in PTRS}) == 0      # nor is any alignment asked
    d.resid_cap = -1
    assert _call(lib, entry, d, dict.fromkeys(PTRS)) == ERR_ARG and b"resid_cap=-1" in lib.million_last_error()
