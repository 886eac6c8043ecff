"""Wide-rank layers on one MI355X: the reference LM at lm_test.py's defaults (2 x MyVMLSTM(650, 650, w_rank=300, u_ranks=300), vocab
10 000, T = 35, dropout 0.5) as a training step (embedding -> layers -> head -> nll -> backward -> clip + SGD) at several batch sizes,
and one layer's forward / backward at B = 20.  Beside it, on the same GPU in the same run: the same Model with lstm_type="custom" (the
package's dense stock-op LSTM) and an eager torch restatement of the VMLMF layer on device tensors (per step: the two low-rank products
per side, the hoisted diagonal terms, the gate math - the reference's own op sequence, fused where torch allows).  Times: device
synchronisation around each timed block, after a warm-up.  One JSON line per case.

    python tools/bench_wide_rank.py [--batches 20,32,64,128] [--iters 10] [--warmup 3]

The kernel list and launches per step come from a separate run under `rocprofv3 --kernel-trace --stats -- python
tools/bench_wide_rank.py --batches 20 --iters 3 --only lm`."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V, H, L, T, RW, RU, P_DROP = 10000, 650, 2, 35, 300, 300, 0.5


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


# ---- eager torch restatement of a V3 layer (MyVMLSTM.lstm_step, vmlmf_lm.py:222-269, with the diagonal terms hoisted) ----------
def eager_params(p):
    H_ = p["u_h"].shape[0]
    ex = (p["dia_x"].reshape(-1).repeat(4) - (p["u_x"].repeat(4, 1) * p["w_x"]).sum(1))
    eh = (p["dia_h"].reshape(-1).repeat(4) - (p["u_h"].repeat(4, 1) * p["w_h"]).sum(1))
    return ex, eh, H_


def eager_layer(p, x, h, c):
    ex, eh, H_ = eager_params(p)
    gxs = torch.matmul(torch.matmul(x, p["u_x"]), p["w_x"].t()) + x.repeat(1, 1, 4) * ex + p["b_x"] + p["b_h"]
    ys = []
    for t in range(x.shape[0]):
        g = gxs[t] + torch.matmul(torch.matmul(h, p["u_h"]), p["w_h"].t()) + h.repeat(1, 4) * eh
        i, f, o, n = g.chunk(4, 1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(n)
        h = torch.sigmoid(o) * torch.tanh(c)
        ys.append(h)
    return torch.stack(ys, 0), h, c


def lm_models(B):
    from vmlmf_amd import Model
    torch.manual_seed(0)
    hip = Model(V, H, L, P_DROP, 0.05, w_rank=RW, u_ranks=[RU], lstm_type="vmlmf").cuda()
    torch.manual_seed(0)
    dense = Model(V, H, L, P_DROP, 0.05, lstm_type="custom").cuda()
    return hip, dense


def lm_step_fn(model, B, nll_loss, optim):
    tok = torch.randint(0, V, (T, B), device="cuda")
    tgt = torch.randint(0, V, (T, B), device="cuda")
    model.train()
    st = [model.state_init(B)]

    def step():
        model.zero_grad()
        states = model.detach(st[0])
        scores, states = model(tok, states)
        loss = nll_loss(scores, tgt)
        loss.backward()
        optim.clip_sgd_step(model.parameters(), lr=1.0, max_norm=0.25)
        st[0] = states
    return step


def eager_lm_step_fn(hip_model, B):
    params = {k: v.detach().clone().requires_grad_(True) for k, v in hip_model.named_parameters()}
    tok = torch.randint(0, V, (T, B), device="cuda")
    tgt = torch.randint(0, V, (T, B), device="cuda")
    drop = torch.nn.Dropout(P_DROP)
    st = [[(torch.zeros(B, H, device="cuda"), torch.zeros(B, H, device="cuda")) for _ in range(L)]]

    def step():
        for p in params.values():
            p.grad = None
        x = drop(params["embed.w"][tok])
        new = []
        for l in range(L):
            p = {k.split(".", 2)[2]: v for k, v in params.items() if k.startswith(f"rnns.{l}.")}
            h0, c0 = (s.detach() for s in st[0][l])
            x, hT, cT = eager_layer(p, x, h0, c0)
            x = drop(x)
            new.append((hT, cT))
        scores = torch.addmm(params["fc.b"], x.view(-1, H), params["fc.w"].t())
        loss = torch.nn.functional.cross_entropy(scores, tgt.reshape(-1)) * B
        loss.backward()
        with torch.no_grad():
            ps = list(params.values())
            torch.nn.utils.clip_grad_norm_(ps, 0.25)
            for q in ps:
                q -= q.grad
        st[0] = new
    return step


def bench_lm(B, iters, warmup):
    from vmlmf_amd import nll_loss, optim
    hip, dense = lm_models(B)
    out = {"case": "lm_train_step", "B": B, "T": T, "H": H, "layers": L, "w_rank": RW, "u_ranks": RU, "vocab": V, "dropout": P_DROP}
    out["ms_hip_vmlmf"] = round(timed(lm_step_fn(hip, B, nll_loss, optim), iters, warmup) * 1e3, 3)
    out["ms_custom_dense"] = round(timed(lm_step_fn(dense, B, nll_loss, optim), iters, warmup) * 1e3, 3)
    out["ms_eager_vmlmf"] = round(timed(eager_lm_step_fn(hip, B), iters, warmup) * 1e3, 3)
    out["speedup_vs_eager"] = round(out["ms_eager_vmlmf"] / out["ms_hip_vmlmf"], 3)
    return out


def bench_layer(B, iters, warmup):
    from vmlmf_amd import MyVMLSTM
    torch.manual_seed(1)
    layer = MyVMLSTM(H, H, w_rank=RW, u_ranks=RU).cuda()
    with torch.no_grad():
        for p in layer.parameters():
            p.uniform_(-0.05, 0.05)
    p = dict(layer.named_parameters())
    x = torch.randn(T, B, H, device="cuda", requires_grad=True)
    h0, c0 = torch.zeros(B, H, device="cuda"), torch.zeros(B, H, device="cuda")
    dy = torch.randn(T, B, H, device="cuda")
    out = {"case": "lm_layer", "B": B, "T": T, "H": H, "w_rank": RW, "u_ranks": RU}

    def hip_fwd():
        with torch.no_grad():
            layer(x, (h0, c0))
    out["ms_hip_fwd"] = round(timed(hip_fwd, iters, warmup) * 1e3, 3)

    def hip_fb():
        y, _ = layer(x, (h0, c0))
        torch.autograd.backward(y, dy)
    out["ms_hip_fwd_bwd"] = round(timed(hip_fb, iters, warmup) * 1e3, 3)

    def eager_fwd():
        with torch.no_grad():
            eager_layer(p, x, h0, c0)
    out["ms_eager_fwd"] = round(timed(eager_fwd, iters, warmup) * 1e3, 3)

    def eager_fb():
        y, _, _ = eager_layer(p, x, h0, c0)
        torch.autograd.backward(y, dy)
    out["ms_eager_fwd_bwd"] = round(timed(eager_fb, iters, warmup) * 1e3, 3)
    out["ms_hip_bwd"] = round(out["ms_hip_fwd_bwd"] - out["ms_hip_fwd"], 3)
    out["ms_eager_bwd"] = round(out["ms_eager_fwd_bwd"] - out["ms_eager_fwd"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="20,32,64,128")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="lm or layer")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    if a.only in ("", "layer"):
        print(json.dumps(bench_layer(20, a.iters, a.warmup)), flush=True)
    if a.only in ("", "lm"):
        for B in (int(b) for b in a.batches.split(",")):
            print(json.dumps(bench_lm(B, a.iters, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
