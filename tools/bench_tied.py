"""What weight tying and word-level embedding dropout cost (Model.tie_weights, Model.embed_dropout; docs/design/lm_tied.md).
  what "grad"    the embedding end of the table's gradient at (R, V, H), element dropout p = 0.5:
                   untied  vmlmf_embed_dropout_backward into a buffer of its own - the step as it is without tying: all of (V, H) written
                   tied    vmlmf_embed_backward_ex with accumulate=1 into a given (V, H) tensor (the head's dW) in place: at most R rows
                   stock   the tied gradient left to autograd: `untied`, then the table-wide add of the two (V, H) gradients
                 and the same three with word dropout 0.5 on the new entry (tied_word; untied / stock have no such form).
  what "gather"  the forward: vmlmf_embed_dropout_forward (p = 0.5) against vmlmf_embed_dropout_forward_ex without and with word
                 dropout 0.5.
  what "step"    loss + backward + clip_sgd_step of the plain PTB network (V 10 000, H 650, 2 VMLMF layers of rank 32, p 0.5) at 32
                 rows of 35 steps: tied against untied.
Every form is captured into a graph of --launches calls; the graphs are replayed in turn, --reps rounds: device-event time per call,
the best of the rounds and the spread (max / min) - bench_actreg.py's method.  No pass / fail gate.  One JSON object per line, appended
to --out (default profiles/lm_tied_bench.jsonl).
`python tools/bench_tied.py [--out FILE] [--reps 9] [--launches 10]`"""
import argparse
import json
import os
import sys

import torch

from bench_distill import alternated_us

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SHAPES = [(1120, 10000, 650), (8960, 10000, 650)]
P = 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_tied_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--launches", type=int, default=10)
    a = ap.parse_args()
    from vmlmf_amd import Model, _lib, optim, unit_gradient
    dev = torch.device("cuda", torch.cuda.current_device())
    one = unit_gradient(dev)
    lib = _lib.lib()
    out = open(a.out, "a")

    def emit(rec, got, base):
        for name, (best, spread) in got.items():
            rec[f"{name}_us"], rec[f"{name}_spread"] = round(best, 2), round(spread, 3)
        for name in got:
            if name != base:
                rec[f"{name}_over_{base}"] = round(got[name][0] / got[base][0], 4)
        rec.update(launches=a.launches, reps=a.reps, device=torch.cuda.get_device_name(0))
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    torch.manual_seed(0)
    for (R, V, H) in SHAPES:
        tok = torch.randint(0, V, (R,), device=dev)
        dy = 1e-3 * torch.randn(R, H, device=dev)
        w = torch.randn(V, H, device=dev)
        head = torch.randn(V, H, device=dev)          # the head's dW of the step
        own = torch.empty(V, H, device=dev)
        y = torch.empty(R, H, device=dev)
        snap = torch.tensor([11, 3], dtype=torch.int64, device=dev)
        nbytes = lib.vmlmf_embed_backward_scratch_bytes(R, V)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        hits = int(torch.unique(tok).numel())

        def untied():
            _lib.check(lib.vmlmf_embed_dropout_backward(R, H, V, _lib.ptr(tok), _lib.ptr(dy), _lib.ptr(own), scratch.data_ptr(), nbytes, P,
                                                        snap.data_ptr(), 0, _lib.raw_stream(dev)))

        def tied(word_p=0.0):
            def body():
                _lib.check(lib.vmlmf_embed_backward_ex(R, H, V, _lib.ptr(tok), _lib.ptr(dy), _lib.ptr(head), 1, scratch.data_ptr(), nbytes, P, word_p,
                                                       snap.data_ptr(), 0, _lib.raw_stream(dev)))
            return body

        def stock():
            untied()
            return head + own

        got = alternated_us({"untied": untied, "tied": tied(), "stock": stock, "tied_word": tied(0.5)}, a.launches, a.reps)
        emit({"what": "grad", "R": R, "V": V, "H": H, "p": P, "rows_hit": hits}, got, "untied")

        def gather_old():
            _lib.check(lib.vmlmf_embed_dropout_forward(R, H, V, _lib.ptr(tok), _lib.ptr(w), _lib.ptr(y), P, snap.data_ptr(), 0, _lib.raw_stream(dev)))

        def gather_ex(word_p):
            def body():
                _lib.check(lib.vmlmf_embed_dropout_forward_ex(R, H, V, _lib.ptr(tok), _lib.ptr(w), _lib.ptr(y), P, word_p, snap.data_ptr(), 0, _lib.raw_stream(dev)))
            return body
        got = alternated_us({"old": gather_old, "ex": gather_ex(0.0), "ex_word": gather_ex(0.5)}, a.launches, a.reps)
        emit({"what": "gather", "R": R, "V": V, "H": H, "p": P}, got, "old")

    V, H, B, T = 10000, 650, 32, 35
    tok, tgt = torch.randint(0, V, (T, B), device=dev), torch.randint(0, V, (T, B), device=dev)

    def step(tie):
        model = Model(V, H, 2, 0.5, 0.05, w_rank=32, u_ranks=[32], lstm_type="vmlmf", tie_weights=tie).to(dev).train()
        model.dropout_state(seed=5)
        params = list(model.parameters())

        def body():
            model.zero_grad(set_to_none=True)
            loss, _ = model.loss(tok, tgt, model.state_init(B))
            loss.backward(one)
            optim.clip_sgd_step(params, 1e-3, 0.25)
        return body
    got = alternated_us({"untied": step(False), "tied": step(True)}, a.launches, a.reps)
    emit({"what": "step", "T": T, "B": B, "H": H, "V": V, "p": 0.5}, got, "untied")
    out.close()


if __name__ == "__main__":
    main()
