"""million_amd — MI355X-native (gfx950) PQ-KV attention hot path of MILLION.

Layout: csrc/ (hand-written HIP kernels + C ABI, built into libmillion_hip.so by `make bindings`),
ops.py (torch tensors -> C ABI), pq_cache.py (host mirror of the reference's DynamicPQCache /
PagedPQCache / PageManager / KernelRegistry), paged_turns.py (extend / extend_request for PagedPQCache with nbits 9 .. 12), train.py (codebook training: the reference's train_pq).  Importing the package does not load the library;
the first op does, and raises if it is missing (no CPU fallback)."""

__all__ = ["ops", "pq_cache", "build", "train"]
