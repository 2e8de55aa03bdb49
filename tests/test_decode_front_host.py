"""What the decode-attention entries of the C ABI share on the host (csrc/million_api.hip: check_fused_append, carve_workspace), without a
GPU: the four entries that take k_new refuse a bad fused append alike, and a fully paged call needs the same workspace whether its
codes are uint8 or wide.  Every call here is refused before a launch: the addresses are made up."""
import ctypes

import pytest

from tests.test_attn_wide_host import A, ERR_ALIGN, ERR_ARG, ERR_WORKSPACE, _desc, lib      # noqa: F401 (lib: the fixture)

# (entry, C of its descriptor, takes an lse argument): the uint8 entries get the twin of the wide descriptor
ENTRIES = [("million_pq_decode_attn_append", 256, False), ("million_pq_decode_attn_lse", 256, True),
           ("million_pq_decode_attn_wide", 1024, True), ("million_pq_decode_attn_packed", 1024, True)]


def _call(lib, entry, has_lse, desc, k_new, v_new, ws_bytes=0):
    """ws_bytes = 0: a call the fused-append checks let through ends at the workspace check, which comes after them."""
    args = [A, k_new, v_new, A + 0x10000, A + 0x20000, A + 0x30000, A + 0x30000, A + 0x40000, A + 0x50000, A + 0x60000, A + 0x70000, A + 0x80000]
    if has_lse:
        args.append(A + 0xd0000)
    return getattr(lib, entry)(ctypes.byref(desc), *args, A + 0x90000, ws_bytes, None)


@pytest.mark.parametrize("entry, C, has_lse", ENTRIES)
def test_fused_append_refusals_are_shared(lib, entry, C, has_lse):
    from million_amd import _lib as L
    err = lib.million_last_error
    k_new, v_new = A + 0xa0000, A + 0xb0000
    d = _desc(L, C=C)
    assert _call(lib, entry, has_lse, d, k_new, None) == ERR_ARG and b"k_new" in err()
    assert _call(lib, entry, has_lse, d, k_new, v_new) == ERR_WORKSPACE      # a good append passes the three checks
    full = _desc(L, C=C, r=128)      # r == resid_cap
    assert _call(lib, entry, has_lse, full, k_new, v_new) == ERR_ARG and b"full window (r=128, cap=128)" in err()
    full.dev_lengths = A + 0xe0000      # the device knows the lengths: not the host's to refuse
    assert _call(lib, entry, has_lse, full, k_new, v_new) == ERR_WORKSPACE and b"full window" not in err()
    for kn, vn in ((k_new + 8, v_new), (k_new, v_new + 8)):
        assert _call(lib, entry, has_lse, d, kn, vn) == ERR_ALIGN and b"k_new / v_new must be 16-byte aligned" in err()
    assert _call(lib, entry, has_lse, full, k_new + 8, v_new) == ERR_ALIGN      # alignment is checked with device lengths too


@pytest.mark.parametrize("bs, nh, nhk, d", [(1, 4, 2, 128), (2, 32, 8, 128), (1, 14, 2, 128),      # nh / nh_k = 7: sized as virtual heads
                                            (300, 16, 8, 128)])                                     # bs * nh_k > 2048: a head of its own
def test_paged_workspace_is_one_size_for_uint8_and_wide(lib, bs, nh, nhk, d):
    from million_amd import _lib as L
    sizes = []
    for C, entry in ((256, lib.million_attn_workspace_bytes), (1024, lib.million_attn_wide_workspace_bytes)):
        x = _desc(L, C=C, nh=nh, nhk=nhk, d=d)
        x.bs = bs
        sizes.append(entry(ctypes.byref(x)))
    assert sizes[0] == sizes[1] > 0, sizes
