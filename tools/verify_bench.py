"""Draft verification (PagedPQCache.verify / commit) per layer, on one cache state, as replayed graphs, interleaved.

  python tools/verify_bench.py [--rounds 15] [--inner 20] [--quick]

Per shape, five graphs of `inner` back-to-back calls each are captured once and replayed in turn, `rounds` times; the figure is the
median replay time over inner (HIP events around the replay):
  heads        verify(route="heads"): one decode launch over the n draft rows as query heads + ops.attn_block_merge
  chunk        verify(route="chunk"): ops.pq_chunk_attn with the rows as chunk + the staging copies (the yardstick's kernel)
  extend       the chunk launch of extend_request alone (host lengths, no staging)
  decode_rows  the decode launch of the heads route alone (nh n query heads)
  decode_1     an ordinary one-token decode launch without append
and for commit: ops.window_commit over 32 layers behind a copy that restores the lengths rows, minus that copy alone, with a
state in which no request flushes and one in which every request does.  One JSON line per shape; profiles/verify_attn.txt keeps
a run.  Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/verify_bench.py --quick`, a run of its own.

  python tools/verify_bench.py --tree [--rounds 15] [--inner 20] [--quick]

Draft trees (verify(tree=) / commit(path=)) at the same shapes, n = 8 and 16 nodes, on a binary tree (node i under (i - 1) // 2)
and on four chains of n / 4 nodes, interleaved with
  linear, linear_again   verify of n rows as a chain, twice: the difference of the two is the run-to-run noise of the comparison
  tree_*                 verify(tree=) of the n nodes: the same decode launch, the block merge under the ancestor masks
  paths_*                what a user without tree= runs: the chain's launches (decode over the rows as heads + block merge)
                         once per root-to-leaf path, on the path's gathered rows
and for commit, over 32 layers with and without a flush: ops.window_commit of 4 rows out of n_bound = 4 (commit(n_accept) after
a chain of 4), out of n_bound = 16, and ops.window_commit(dev_rows=) of a 4-node path out of 16 (commit(path=)), each minus the
copy that restores the lengths rows.  profiles/verify_tree.txt keeps a run."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402

from million_amd import ops  # noqa: E402
from million_amd.pq_cache import PagedPQCache  # noqa: E402

D, C, PS, CAP, R, RS = 128, 256, 64, 128, 77, 100
MODELS = {"llama-3.1-8b": dict(nh=32, nhk=8, M=64, T=32768, ns=(2, 4, 8, 16)),
          "llama-2-7b": dict(nh=32, nhk=32, M=64, T=4096, ns=(4, 8, 16))}


def _cache(bs, nh, nhk, M, layers, T, r, rs, max_tokens):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    cache = PagedPQCache(bs=bs, nh=nh, num_key_value_heads=nhk, M=M, layer_num=layers, d=D, page_size=PS,
                         extended_residual_size=CAP, max_tokens=max_tokens)
    cache.set_cent(torch.randn(M, C, D // M, device=dev, generator=g).half(), torch.randn(M, C, D // M, device=dev, generator=g).half())
    # the state is written, not computed: random codes in every page, random window rows, the lengths of a request T tokens in
    cache.key_page_pool.copy_(torch.randint(0, C, cache.key_page_pool.shape, device=dev, dtype=torch.uint8, generator=g))
    cache.value_page_pool.copy_(torch.randint(0, C, cache.value_page_pool.shape, device=dev, dtype=torch.uint8, generator=g))
    cache._kres_all.copy_(torch.randn(cache._kres_all.shape, device=dev, generator=g).half())
    cache._vres_all.copy_(torch.randn(cache._vres_all.shape, device=dev, generator=g).half())
    cache._T_a[:], cache._r_a[:], cache._rs_a[:], cache._seen_a[:] = T, r, rs, T + r
    for l in range(layers):
        cache._sync_lengths(l)
    return cache, g


def _graph(fn, inner):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(inner):
            fn()
    gr.replay()
    torch.cuda.synchronize()
    return gr


def _interleaved_us(graphs, rounds, inner):
    """{name: median us per call}: the graphs replayed in turn, `rounds` times."""
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, gr in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            gr.replay()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3 / inner)
    med = lambda v: sorted(v)[len(v) // 2]
    return {k: round(med(v), 2) for k, v in times.items()}, {k: round(max(v) - min(v), 2) for k, v in times.items()}


def run_attention(model, n, rounds, inner, bs=1):
    m = MODELS[model]
    nh, nhk, M, T = m["nh"], m["nhk"], m["M"], m["T"]
    cache, g = _cache(bs, nh, nhk, M, 1, T, R, RS, T + 1024)
    dev = cache.device
    q = torch.randn(bs, nh, n, D, device=dev, generator=g).half()
    k = torch.randn(bs, nhk, n, D, device=dev, generator=g).half()
    v = torch.randn(bs, nhk, n, D, device=dev, generator=g).half()
    q1 = q[:, :, :1].contiguous()
    qh = q.view(bs, nh * n, 1, D)
    ids, kres, vres, dl = cache.page_ids[0], cache.key_residual_cache[0], cache.value_residual_cache[0], cache.lengths[0]
    kw = dict(M=M, C=C, k_page_ids=ids, v_page_ids=ids, page_size=PS)
    pools = (cache.key_page_pool, cache.value_page_pool, cache._kprep, cache._vprep, kres, vres)
    ws1 = torch.zeros(ops.decode_workspace_bytes(q1, kres, nh_k=nhk, M=M, C=C), dtype=torch.uint8, device=dev)
    wsn = torch.zeros(ops.decode_workspace_bytes(qh, kres, nh_k=nhk, M=M, C=C), dtype=torch.uint8, device=dev)
    fns = {
        "heads": lambda: cache.verify(q, k, v, 0, route="heads"),
        "chunk": lambda: cache.verify(q, k, v, 0, route="chunk"),
        "extend": lambda: ops.pq_chunk_attn(q, k, v, *pools, R, n_tokens=T, resid_start=RS, **kw),
        "decode_rows": lambda: ops.pq_decode_attn(qh, *pools, R, n_tokens=cache.max_tokens, dev_lengths=dl, workspace=wsn, return_lse=True, **kw),
        "decode_1": lambda: ops.pq_decode_attn(q1, *pools, R, n_tokens=cache.max_tokens, dev_lengths=dl, workspace=ws1, **kw),
    }
    oh, oc = fns["heads"]().float(), fns["chunk"]().float()
    torch.cuda.synchronize()
    rel = ((oh - oc).norm() / oc.norm()).item()
    graphs = {name: _graph(fn, inner) for name, fn in fns.items()}
    us, spread = _interleaved_us(graphs, rounds, inner)
    faults = ops.tail_faults()
    assert faults == 0, f"{faults} split merges gave up"
    return dict(model=model, bs=bs, nh=nh, nh_k=nhk, G=nh // nhk, M=M, T=T, r=R, n=n, rows_per_kv_head=n * nh // nhk, us=us,
                spread_us=spread, heads_over_chunk=round(us["heads"] / us["chunk"], 3), block_merge_us=round(us["heads"] - us["decode_rows"], 2),
                rel_heads_vs_chunk=float(f"{rel:.2e}"))


def run_commit(rounds, inner, layers=32, bs=1, nh=32, nhk=8, M=64, n=4):
    out = {}
    for tag, r in (("no_flush", 40), ("flush", CAP - 2)):
        cache, g = _cache(bs, nh, nhk, M, layers, 4096, r, RS, 8192)
        dev = cache.device
        shape = (layers, bs, nhk, 16, D)
        ks, vs = torch.randn(shape, device=dev, generator=g).half(), torch.randn(shape, device=dev, generator=g).half()
        dev_n = torch.full((bs,), n, dtype=torch.int32, device=dev)
        saved = cache._lengths_all.clone()

        def reset():
            cache._lengths_all.copy_(saved)

        def commit():
            reset()
            ops.window_commit(ks, vs, cache._kres_all, cache._vres_all, cache._kprep, cache._vprep, cache.key_page_pool,
                              cache.value_page_pool, cache._page_ids_all, cache._lengths_all, dev_n, M=M, C=C, n_bound=n)
        graphs = {"commit": _graph(commit, inner), "reset": _graph(reset, inner)}
        us, spread = _interleaved_us(graphs, rounds, inner)
        graphs["commit"].replay()
        torch.cuda.synchronize()
        moved = cache._lengths_all[0, 0].tolist()
        out[tag] = dict(r=r, n_accept=n, us=us, spread_us=spread, window_commit_us=round(us["commit"] - us["reset"], 2), lengths_after=moved)
    return dict(commit=True, layers=layers, bs=bs, nh_k=nhk, M=M, **out)


def _tree_shapes(n):
    binary = [(i - 1) // 2 if i else -1 for i in range(n)]
    chains = [-1 if i % (n // 4) == 0 else i - 1 for i in range(n)]
    return {"binary": binary, "chains4": chains}


def _leaf_paths(parents):
    from million_amd import spec_tree
    leaves = [i for i in range(len(parents)) if i not in parents]
    return [spec_tree.chain_of(parents, i) for i in leaves]


def run_tree_attention(model, n, rounds, inner, bs=1):
    m = MODELS[model]
    nh, nhk, M, T = m["nh"], m["nhk"], m["M"], m["T"]
    cache, g = _cache(bs, nh, nhk, M, 1, T, R, RS, T + 1024)
    dev = cache.device
    q = torch.randn(bs, nh, n, D, device=dev, generator=g).half()
    k = torch.randn(bs, nhk, n, D, device=dev, generator=g).half()
    v = torch.randn(bs, nhk, n, D, device=dev, generator=g).half()
    ids, kres, vres, dl = cache.page_ids[0], cache.key_residual_cache[0], cache.value_residual_cache[0], cache.lengths[0]
    kw = dict(M=M, C=C, k_page_ids=ids, v_page_ids=ids, page_size=PS)
    pools = (cache.key_page_pool, cache.value_page_pool, cache._kprep, cache._vprep, kres, vres)
    route = cache._verify_route(n)
    trees = _tree_shapes(n)
    keep = []      # the records (dev_n, masks) a captured graph reads: verify() starts a new one when the tree changes

    def chain_launches(rows):
        """The launches of verify(route="heads") of a chain, on gathered rows, without the cache's host side."""
        qc, kc, vc = q[:, :, rows].contiguous(), k[:, :, rows].contiguous(), v[:, :, rows].contiguous()
        qh = qc.view(bs, nh * len(rows), 1, D)
        ws = torch.zeros(ops.decode_workspace_bytes(qh, kres, nh_k=nhk, M=M, C=C), dtype=torch.uint8, device=dev)
        dn = torch.full((bs,), len(rows), dtype=torch.int32, device=dev)
        ks, vs = cache._kstage[0], cache._vstage[0]

        def fn():
            oa, la = ops.pq_decode_attn(qh, *pools, R, n_tokens=cache.max_tokens, dev_lengths=dl, workspace=ws, return_lse=True, **kw)
            oa, la = oa.view(bs, nh, len(rows), D), la.view(bs, nh, len(rows))
            return ops.attn_block_merge(qc, kc, vc, oa, la, dn, out=oa, k_stage=ks, v_stage=vs)
        return fn

    def graph_of(fn):
        for _ in range(3):
            fn()
        keep.append(cache._verify_rec)
        return _graph(fn, inner)

    fns = {"linear": lambda: cache.verify(q, k, v, 0, route=route), "linear_again": lambda: cache.verify(q, k, v, 0, route=route)}
    for name, parents in trees.items():
        fns["tree_" + name] = (lambda parents: lambda: cache.verify(q, k, v, 0, route=route, tree=parents))(parents)
    # the result of the tree's verify against the chain's launches on every leaf path, before anything is timed
    worst = 0.0
    for name, parents in trees.items():
        out = fns["tree_" + name]().float()
        for path in _leaf_paths(parents):
            lin = chain_launches(path)().float()
            worst = max(worst, ((out[:, :, path] - lin).norm() / lin.norm()).item())
    torch.cuda.synchronize()
    graphs = {name: graph_of(fn) for name, fn in fns.items()}
    n_paths = {}
    for name, parents in trees.items():
        per_path = [chain_launches(path) for path in _leaf_paths(parents)]
        n_paths[name] = len(per_path)
        graphs["paths_" + name] = _graph((lambda per_path: lambda: [f() for f in per_path])(per_path), inner)
    us, spread = _interleaved_us(graphs, rounds, inner)
    faults = ops.tail_faults()
    assert faults == 0, f"{faults} split merges gave up"
    return dict(tree=True, model=model, bs=bs, nh=nh, nh_k=nhk, M=M, T=T, r=R, n=n, route=route, leaf_paths=n_paths, us=us, spread_us=spread,
                noise_us=round(abs(us["linear"] - us["linear_again"]), 2),
                tree_minus_linear_us={name: round(us["tree_" + name] - us["linear"], 2) for name in trees},
                paths_over_tree={name: round(us["paths_" + name] / us["tree_" + name], 2) for name in trees},
                rel_tree_vs_paths=float(f"{worst:.2e}"))


def run_tree_commit(rounds, inner, layers=32, bs=1, nh=32, nhk=8, M=64, a=4, path=(0, 2, 5, 11)):
    out = {}
    for tag, r in (("no_flush", 40), ("flush", CAP - 2)):
        cache, g = _cache(bs, nh, nhk, M, layers, 4096, r, RS, 8192)
        dev = cache.device
        shape = (layers, bs, nhk, 16, D)
        ks, vs = torch.randn(shape, device=dev, generator=g).half(), torch.randn(shape, device=dev, generator=g).half()
        dev_n = torch.full((bs,), a, dtype=torch.int32, device=dev)
        rows = torch.zeros(bs, 16, dtype=torch.int32, device=dev)
        rows[:, :a] = torch.tensor(path, dtype=torch.int32, device=dev)
        saved = cache._lengths_all.clone()

        def reset():
            cache._lengths_all.copy_(saved)

        def commit(n_bound, **kw):
            def fn():
                reset()
                ops.window_commit(ks, vs, cache._kres_all, cache._vres_all, cache._kprep, cache._vprep, cache.key_page_pool,
                                  cache.value_page_pool, cache._page_ids_all, cache._lengths_all, dev_n, M=M, C=C, n_bound=n_bound, **kw)
            return fn
        graphs = {"commit_of_4": _graph(commit(a), inner), "commit_of_16": _graph(commit(16), inner),
                  "commit_of_16_again": _graph(commit(16), inner), "commit_rows_of_16": _graph(commit(16, dev_rows=rows), inner),
                  "reset": _graph(reset, inner)}
        us, spread = _interleaved_us(graphs, rounds, inner)
        graphs["commit_rows_of_16"].replay()
        torch.cuda.synchronize()
        out[tag] = dict(r=r, n_accept=a, path=list(path), us=us, spread_us=spread, noise_us=round(abs(us["commit_of_16"] - us["commit_of_16_again"]), 2),
                        rows_minus_linear_us=round(us["commit_rows_of_16"] - us["commit_of_16"], 2),
                        window_commit_rows_us=round(us["commit_rows_of_16"] - us["reset"], 2), lengths_after=cache._lengths_all[0, 0].tolist())
    return dict(tree=True, commit=True, layers=layers, bs=bs, nh_k=nhk, M=M, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="one attention shape and the commit rows")
    ap.add_argument("--tree", action="store_true", help="draft trees: verify(tree=) and commit(path=) against the chain's calls")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "verify_bench needs the GPU (no CPU timing)"
    if a.tree:
        shapes = [(model, n) for model in MODELS for n in (8, 16)]
        for model, n in shapes[:1] if a.quick else shapes:
            print(json.dumps(run_tree_attention(model, n, a.rounds, a.inner)), flush=True)
        print(json.dumps(run_tree_commit(a.rounds, a.inner)), flush=True)
        return
    shapes = [(model, n) for model, m in MODELS.items() for n in m["ns"]]
    if a.quick:
        shapes = shapes[1:2]
    for model, n in shapes:
        print(json.dumps(run_attention(model, n, a.rounds, a.inner)), flush=True)
    print(json.dumps(run_commit(a.rounds, a.inner)), flush=True)


if __name__ == "__main__":
    main()
