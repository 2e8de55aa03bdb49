"""SharedPrefix: several continuation requests decode against ONE frozen prompt that is read once per step.

`fork` gives every continuation a slot of its own whose page table names the prompt's pages: the pages are shared, but a
decode launch still streams the whole prompt from HBM once per forked slot.  Here the prompt stays in one slot of a
PagedPQCache (the prefix cache) and the continuations live in the slots of a second PagedPQCache; a step of a layer is three
launches:

  1. ops.pq_chunk_attn: the n continuations' queries as the n_q = n query rows of ONE request against the prefix slot - its
     codes and its window are read once for all of them - with the rows' log-sum-exp;
  2. the continuation cache's own decode step (fused append, flush when its window is full), with its log-sum-exp;
  3. ops.attn_merge of the two partial attentions over the disjoint key sets, written into the second's output.

What differs from fork + batched decode: the prefix is FROZEN while the object lives.  Its window rows stay fp16 for good,
where a forked slot's copy of them is encoded as its decoding goes on; the two routes therefore do not give the same bits, and
neither is the other's reference.  Whether the shared route is faster depends on the prompt length and the number of
continuations (tools/shared_prefix_bench.py)."""
from __future__ import annotations

import torch

from . import ops


class SharedPrefix:
    def __init__(self, prefix_cache, slot, cont_cache):
        """prefix_cache / slot: the PagedPQCache slot that holds the shared prompt (prefilled, possibly decoded a few steps:
        codes and window both count).  cont_cache: the PagedPQCache of the continuations, one per slot, with an ordinary
        life: decode, flush, extend_request, release.  Both caches must agree in heads, d, M, C, device and codebooks; the
        prefix slot must be between steps (the same rule as fork: every layer at the same lengths, no encode-ahead pending)."""
        p, c = prefix_cache, cont_cache
        if getattr(p, "sink_tokens", 0) or getattr(c, "sink_tokens", 0):
            raise NotImplementedError("SharedPrefix: caches with sink_tokens > 0 are not served yet (DESIGN.md 4.13)")
        for x in (p, c):
            if getattr(x, "nbits", 8) > 8:
                raise NotImplementedError(f"SharedPrefix: caches with nbits={x.nbits} (uint16 codes) are not served yet (DESIGN.md 4.14)")
        slot = int(slot)
        if not 0 <= slot < p.bs:
            raise RuntimeError(f"SharedPrefix: slot {slot} outside [0, {p.bs})")
        for name in ("nh", "num_key_value_heads", "d", "M", "C", "layer_num"):
            if getattr(p, name) != getattr(c, name):
                raise RuntimeError(f"SharedPrefix: the caches differ in {name} ({getattr(p, name)} / {getattr(c, name)})")
        if p.device != c.device:
            raise RuntimeError(f"SharedPrefix: the caches are on different devices ({p.device} / {c.device})")
        if p._cent_digests() != c._cent_digests():
            raise RuntimeError("SharedPrefix: the caches have different codebooks")
        cols = (p._T_a[:, slot], p._r_a[:, slot], p._rs_a[:, slot])
        if p._ahead is not None or any((x != x[0]).any() for x in cols):
            raise RuntimeError("SharedPrefix: the prefix slot is mid-step (its layers are at different lengths, or encode-ahead "
                               "work is pending); build it between steps")
        if p._pre_join:      # an encode-ahead launch of the finished step may still run on the side stream: it writes pages past T only
            torch.cuda.current_stream().wait_stream(p._side)
        self.prefix, self.slot, self.cont = p, slot, c
        self.T, self.r, self.resid_start = int(cols[0][0]), int(cols[1][0]), int(cols[2][0])
        self._bufs = {}      # per (kind, layer): what a call keeps between steps

    def _check_frozen(self):
        p, s = self.prefix, self.slot
        if ((p._T_a[:, s] != self.T).any() or (p._r_a[:, s] != self.r).any() or (p._rs_a[:, s] != self.resid_start).any()):
            raise RuntimeError(f"SharedPrefix: slot {s} of the prefix cache has moved since this object was built "
                               f"(it was at T={self.T}, r={self.r}, resid_start={self.resid_start}); the prefix is frozen")

    def _prefix_attn(self, q_rows, layer_idx, key):
        """q_rows (1, nh, n, d), any row strides: (out (1, nh, n, d), lse (1, nh, n)) of the rows over the prefix slot alone."""
        p, s = self.prefix, self.slot
        n = q_rows.shape[2]
        buf = self._bufs.get(key)
        if buf is None or buf[0].shape[2] != n:
            out = torch.empty(1, n, p.nh, p.d, dtype=torch.float16, device=p.device).transpose(1, 2)
            lse = torch.empty(1, p.nh, n, dtype=torch.float32, device=p.device)
            ids = p.page_ids[layer_idx][s:s + 1]
            desc = ops.chunk_attn_desc(q_rows, p.key_residual_cache[layer_idx][s:s + 1], nh_k=p.num_key_value_heads, M=p.M, C=p.C,
                                       n_tokens=self.T, r=self.r, n_c=0, resid_start=self.resid_start, k_paged=True, v_paged=True,
                                       page_size=p.page_size, n_pages_cap=ids.shape[2], out=out)
            need = ops.chunk_attn_workspace_bytes(desc)
            ws = torch.empty(max(need, 1), dtype=torch.uint8, device=p.device)
            buf = self._bufs[key] = (out, lse, ws)
        out, lse, ws = buf
        ids = p.page_ids[layer_idx][s:s + 1]
        return ops.pq_chunk_attn(q_rows, None, None, p.key_page_pool, p.value_page_pool, p._kprep, p._vprep,
                                 p.key_residual_cache[layer_idx][s:s + 1], p.value_residual_cache[layer_idx][s:s + 1], self.r,
                                 M=p.M, C=p.C, n_tokens=self.T, resid_start=self.resid_start, k_page_ids=ids, v_page_ids=ids,
                                 page_size=p.page_size, out=out, workspace=ws, lse=lse)

    def decoding(self, q, k, v, layer_idx, use_dev_lengths=False):
        """One decode step of one layer for every continuation: q (n, nh, 1, d), k / v (n, nh_k, 1, d), n = cont.bs.  Returns
        (n, nh, 1, d): each continuation's attention over [the prefix's codes and window; its own codes and window; its new
        row], which is appended to its window (cont.decoding_with_pages).  The returned tensor is reused by the next call of
        the layer; after the first call of a layer nothing is allocated."""
        self._check_frozen()
        c = self.cont
        if q.dim() != 4 or q.shape[0] != c.bs or q.shape[2] != 1 or not q.is_contiguous():
            raise RuntimeError(f"SharedPrefix.decoding: q must be contiguous ({c.bs}, nh, 1, d)")
        o1, l1 = self._prefix_attn(q.permute(2, 1, 0, 3), layer_idx, ("dec", layer_idx))      # the n requests as n_q = n rows of batch 1
        buf = self._bufs.get(("dec2", layer_idx))
        if buf is None:
            buf = self._bufs[("dec2", layer_idx)] = (torch.empty_like(q),
                                                     torch.empty(c.bs, c.nh, 1, dtype=torch.float32, device=q.device))
        o2, l2 = c.decoding_with_pages(q, k, v, layer_idx, out=buf[0], use_dev_lengths=use_dev_lengths, lse=buf[1])
        return ops.attn_merge([o1.permute(2, 1, 0, 3), o2], [l1.permute(2, 1, 0), l2], out=o2)

    def extend_request(self, b, q, k, v, layer_idx):
        """A block of n new tokens of continuation b (a question asked of the document): q (1, nh, n, d), k / v
        (1, nh_k, n, d).  Returns (1, nh, n, d): each row's attention over [the prefix; the continuation's codes and window;
        the block, causally]; the block is stored as cont.extend_request stores it."""
        self._check_frozen()
        if q.dim() != 4 or q.shape[0] != 1:
            raise RuntimeError("SharedPrefix.extend_request: tensors of batch 1")
        o1, l1 = self._prefix_attn(q, layer_idx, ("ext", layer_idx))
        o2, l2 = self.cont.extend_request(b, q, k, v, layer_idx, return_lse=True)
        return ops.attn_merge([o1, o2], [l1, l2], out=o2)
