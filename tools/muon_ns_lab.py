#!/usr/bin/env python
"""Time Muon.step_ with ns_dtype "bfloat16" and "float32" on the C2 ViT layout (D 128, mlp 256,
4 layers, 200 classes: nine routed matrices, 128 x 256 / 256 x 128 / 128 x 200).

Each optimizer's step_ is captured once in a hipGraph (the way the engines run it) and replayed; both
are timed in ONE process, alternating: ``--rounds`` rounds, in each round ``--replays`` back-to-back
replays of one graph between two device events, then the same for the other.  Reported per variant:
the median over rounds of the per-replay time, and min / max.  ``ns_chain_f32`` is the fp32
Newton-Schulz launches alone (3 x ns_steps, csrc/muon_ns_f32.hip), the figure to hold against
DESIGN.md §5.3's one-CU estimate.  Prints one JSON line.

    python tools/muon_ns_lab.py [--rounds 30] [--replays 200] [--warmup 50]
"""
import argparse
import json
import os
import statistics
import sys
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    args = ap.parse_args()

    import torch
    from plaincv_amd.models.vit_small import VisionTransformer
    from plaincv_amd.optim.muon import Muon
    from plaincv_amd.params import ParamStore
    if not torch.cuda.is_available():
        raise SystemExit("muon_ns_lab: no GPU visible (timings need the device)")
    dev = torch.device("cuda:0")
    lay = VisionTransformer(num_classes=200, patch_size=4, hidden_size=128, mlp_dim=256, num_layers=4,
                            num_heads=4).layout((64, 64, 64, 3))
    gen = torch.Generator().manual_seed(0)
    init = OrderedDict((k, 0.1 * torch.randn(l.shape, generator=gen)) for k, l in lay.leaves.items())
    grads = OrderedDict((k, 0.01 * torch.randn(l.shape, generator=gen)) for k, l in lay.leaves.items())
    gs = torch.full((1,), 0.5, device=dev)
    stream = torch.cuda.Stream(device=dev)

    def capture(fn):
        fn()                                   # eager once: loads the kernels
        torch.cuda.synchronize()
        stream.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            fn()
        return g

    graphs, routed = OrderedDict(), None
    for dt in ("bfloat16", "float32"):
        tx = Muon(1e-3, weight_decay=0.01, ns_dtype=dt)
        store = ParamStore(lay, dev)
        store.load(init)
        store.zero_grad()
        for k, v in grads.items():
            store.grads[k].copy_(v.to(dev))
        st = tx.init(store)
        routed = [tuple(store.params[k].shape) for k in st.routed]
        graphs[f"step_{dt}"] = capture(lambda tx=tx, store=store, st=st: tx.step_(store, st, gscale=gs))
        if dt == "float32":
            graphs["ns_chain_f32"] = capture(lambda tx=tx, st=st: tx._ns_f32(st))
            ws_bytes = st.ns_ws.numel() * 4
            tiles = (st.ns_nsym, st.ns_nupd)

    times = {k: [] for k in graphs}
    with torch.cuda.stream(stream):
        for g in graphs.values():
            for _ in range(args.warmup):
                g.replay()
        stream.synchronize()
        for _ in range(args.rounds):
            for name, g in graphs.items():     # alternating: one window per variant per round
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(args.replays):
                    g.replay()
                e1.record(stream)
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / args.replays)
    out = {"tool": "muon_ns_lab", "device": torch.cuda.get_device_name(0), "layout": "vit_c2", "routed": routed,
           "rounds": args.rounds, "replays": args.replays, "f32_workspace_bytes": ws_bytes,
           "f32_tiles_sym_upd": tiles, "us": {}}
    for name, t in times.items():
        out["us"][name] = {"median": round(statistics.median(t), 2), "min": round(min(t), 2), "max": round(max(t), 2)}
    out["step_ratio_f32_over_bf16"] = round(out["us"]["step_float32"]["median"] / out["us"]["step_bfloat16"]["median"], 3)
    out["one_cu_estimate_us"] = 195.0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
