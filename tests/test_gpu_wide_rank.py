"""GPU: layers at wide ranks (padded w_rank > 32 or padded hidden rank > 128, up to the LM's default 300 / 300) on the
step-wise path with the rank-agnostic x side and weight gradients (vmlmf_generic.hip: wide_xproj, wide_dqx_dx, wide_wgrad),
against the oracle, the reference's goldens and themselves (determinism).  Tolerances: tests/hip_util.py."""
import numpy as np
import pytest
import torch

import vmlmf_oracle as O
from conftest import load_golden
from hip_util import ORDER, run_hip, run_literal, compare_all, assert_out, assert_grad

pytestmark = pytest.mark.gpu
DEV = "cuda"

GROUPED = (O.V2, O.V4, O.V6)

CASES = [
    # variant, B, T, I, H, rw, ru, time_major, with_state, need_dx
    (O.V1, 5, 7, 77, 180, 64, [64], False, True, True),          # OPP-like cell, KX 64
    (O.V1, 1, 1, 40, 144, 40, [144], False, False, True),        # B = T = 1, G KH 144
    (O.V1, 33, 6, 136, 200, 136, [37], True, True, False),       # KX 136, odd u_rank
    (O.V1, 300, 3, 50, 70, 43, [41], False, False, True),        # B = 300, ranks not multiples of 16
    (O.V2, 4, 9, 64, 180, 40, [48, 40], False, True, True),      # G KH 176
    (O.V2, 7, 5, 70, 300, 64, [150, 150], True, False, True),    # G KH 608
    (O.V3, 6, 11, 304, 304, 300, [300], True, True, True),       # KX 304, KH 304
    (O.V3, 2, 40, 96, 96, 64, [90], False, True, True),          # batch-first LM layer, T = 40
    (O.V4, 9, 4, 160, 160, 64, [72, 60], True, True, True),      # flat layout, G KH 288
    (O.V4, 2, 3, 200, 200, 136, [100, 100], False, False, True),  # V4 at B = 2 (the reference squeezes B = 1 away)
    (O.V5, 5, 6, 100, 180, 64, [150], False, True, True),        # per-gate tensors, KH 152
    (O.V5, 3, 4, 304, 160, 300, [40], True, False, True),        # more inputs than units, KX 304
    (O.V6, 4, 5, 100, 180, 64, [60, 60], False, True, True),     # (f,i,n,o) on both sides, G KH 256
    (O.V6, 6, 3, 40, 96, 37, [48, 44], True, True, False),       # odd w_rank
]


def _case_io(case):
    variant, B, T, I, H, rw, ru, tm, with_state, _ = case
    rng = np.random.Generator(np.random.PCG64(2000 + B + 7 * T + 13 * H + rw))
    P = O.make_params(variant, I, H, rw, ru if variant in GROUPED else ru[0], seed=H + rw)
    shp = (T, B, I) if tm else (B, T, I)
    x = rng.standard_normal(shp).astype(np.float32)
    h0 = (0.4 * rng.standard_normal((B, H))).astype(np.float32) if with_state else None
    c0 = (0.4 * rng.standard_normal((B, H))).astype(np.float32) if with_state else None
    dy = rng.standard_normal(shp[:2] + (H,)).astype(np.float32)
    dhT = rng.standard_normal((B, H)).astype(np.float32)
    dcT = rng.standard_normal((B, H)).astype(np.float32)
    return P, x, h0, c0, dy, dhT, dcT


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"v{c[0]}_B{c[1]}_T{c[2]}_I{c[3]}_H{c[4]}_r{c[5]}_{'x'.join(map(str, c[6]))}"
                                                      f"{'_tm' if c[7] else ''}{'_dx' if c[9] else ''}")
def test_wide_seeded_shapes_vs_oracle(case):
    variant, tm, need_dx = case[0], case[7], case[9]
    P, x, h0, c0, dy, dhT, dcT = _case_io(case)
    got = run_hip(variant, P, x, h0, c0, dy, dhT, dcT, time_major=tm, need_dx=need_dx)
    ref = run_literal(variant, P, x, h0, c0, dy, dhT, dcT, time_major=tm)
    compare_all(got, ref, f"wide.v{variant}")


def test_wide_inference_forward_matches_training_forward():
    """The inference call (no reserve) runs the same x-side GEMMs into the workspace: same outputs, bit for bit."""
    from vmlmf_amd import vmlmf_sequence
    case = CASES[6]
    variant, tm = case[0], case[7]
    P, x, h0, c0, *_ = _case_io(case)
    params = [torch.tensor(np.asarray(P[k]), device=DEV) for k in ORDER[variant]]
    xt, h0t, c0t = (torch.tensor(a, device=DEV) for a in (x, h0, c0))
    rw, ru = case[5], case[6]
    with torch.no_grad():
        y_inf = vmlmf_sequence(variant, xt, h0t, c0t, params, rw, ru, time_major=tm)[0]
    y_tr = vmlmf_sequence(variant, xt, h0t, c0t, [p.clone().requires_grad_(True) for p in params], rw, ru, time_major=tm)[0]
    assert torch.equal(y_inf, y_tr.detach())


def test_wide_training_call_is_bit_identical_run_to_run():
    case = CASES[8]
    variant, tm = case[0], case[7]
    P, x, h0, c0, dy, dhT, dcT = _case_io(case)
    a = run_hip(variant, P, x, h0, c0, dy, dhT, dcT, time_major=tm)
    b = run_hip(variant, P, x, h0, c0, dy, dhT, dcT, time_major=tm)
    for k in ("y", "hT", "cT", "dx", "dh0", "dc0"):
        assert np.array_equal(a[k], b[k]), k
    for k in a["G"]:
        assert np.array_equal(a["G"][k], b["G"][k]), k


# ---- the reference's goldens (tools/make_golden_wide_rank.py) ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wide_cell_v1", "wide_seq_v1", "wide_seq_v2", "wide_seq_v5", "wide_seq_v6"])
def test_wide_har_vs_reference_golden(name):
    d = load_golden(name)
    variant, B, T = (int(v) for v in d["meta"][:3])
    if T == 1:   # bare cell: one step from the golden (h, c)
        got = run_hip(variant, d["P"], d["x"][:, None, :], d["h0"], d["c0"], None, d["dh"], d["dc"])
        assert_out(got["hT"], d["h1"], "h1")
        assert_out(got["cT"], d["c1"], "c1")
        assert_grad(got["dx"][:, 0, :], d["dx"], "dx")
        assert_grad(got["dh0"], d["dh0"], "dh0")
        assert_grad(got["dc0"], d["dc0"], "dc0")
    else:
        got = run_hip(variant, d["P"], d["x"], None, None, d["dy"], d["dhT"], None)
        assert_out(got["y"], d["y"], "y")
        assert_out(got["hT"], d["hT"], "hT")
        assert_grad(got["dx"], d["dx"], "dx")
    for k, v in d["G"].items():
        assert_grad(got["G"][k], v, "G." + k)


@pytest.mark.parametrize("name", ["wide_lm_v3", "wide_lm_v4"])
def test_wide_lm_layer_vs_reference_golden(name):
    d = load_golden(name)
    variant = int(d["meta"][0])
    got = run_hip(variant, d["P"], d["x"], d["h0"], d["c0"], d["dy"], d["dhT"], d["dcT"], time_major=True)
    for k in ("y", "hT", "cT"):
        assert_out(got[k], d[k], k)
    for k in ("dx", "dh0", "dc0"):
        assert_grad(got[k], d[k], k)
    for k, v in d["G"].items():
        assert_grad(got["G"][k], v, "G." + k)


# ---- the reference LM at its own defaults (lm_test.py: hidden 650, wRank 300, uRanks 300) -------------------------------------
def test_reference_lm_layer_full_size_vs_unified_oracle():
    """MyVMLSTM(650, 650, w_rank=300, u_ranks=300), B = 20, T = 35, non-zero states and dhT / dcT, against the fp64 oracle."""
    B, T, H, rw, ru = 20, 35, 650, 300, 300
    rng = np.random.Generator(np.random.PCG64(650))
    P = O.make_params(O.V3, H, H, rw, ru, seed=11, scale=0.05)
    x = rng.standard_normal((T, B, H)).astype(np.float32)
    h0 = (0.3 * rng.standard_normal((B, H))).astype(np.float32)
    c0 = (0.3 * rng.standard_normal((B, H))).astype(np.float32)
    dy = rng.standard_normal((T, B, H)).astype(np.float32)
    dhT = rng.standard_normal((B, H)).astype(np.float32)
    dcT = rng.standard_normal((B, H)).astype(np.float32)
    got = run_hip(O.V3, P, x, h0, c0, dy, dhT, dcT, time_major=True)
    y, hT, cT, dx, dh0, dc0, G = O.unified_run(O.V3, P, x, h0, c0, dy, dhT, dcT)
    assert_out(got["y"], y, "y")
    assert_out(got["hT"], hT, "hT")
    assert_out(got["cT"], cT, "cT")
    assert_grad(got["dx"], dx, "dx")
    assert_grad(got["dh0"], dh0, "dh0")
    assert_grad(got["dc0"], dc0, "dc0")
    for k, v in G.items():
        assert_grad(got["G"][k], v, "G." + k)


def _lm_model(dropout, seed=0):
    from vmlmf_amd import Model
    torch.manual_seed(seed)
    return Model(10000, 650, 2, dropout=dropout, winit=0.05, w_rank=300, u_ranks=[300], lstm_type="vmlmf")


def test_reference_lm_network_two_minibatches_vs_literal():
    """The lm_test.py loop at its defaults: Model -> nll_loss -> backward -> clip_sgd_step, two minibatches with state carry,
    against the oracle's literal Model.forward under host autograd (fp64), with the stock clip + SGD step."""
    from vmlmf_amd import nll_loss, optim
    B, T, L = 20, 35, 2
    model = _lm_model(0.0)
    ref = {k: v.detach().double().clone().requires_grad_(True) for k, v in model.named_parameters()}
    model = model.to(DEV)
    rng = np.random.Generator(np.random.PCG64(35))
    states = model.state_init(B)
    rstates = [(torch.zeros(B, 650, dtype=torch.float64), torch.zeros(B, 650, dtype=torch.float64)) for _ in range(L)]
    for i in range(2):
        tok = rng.integers(0, 10000, size=(T, B))
        tgt = rng.integers(0, 10000, size=(T, B))
        model.zero_grad()
        states = model.detach(states)
        scores, states = model(torch.tensor(tok, device=DEV), states)
        loss = nll_loss(scores, torch.tensor(tgt, device=DEV))
        loss.backward()
        for p in ref.values():
            p.grad = None
        rscores, rstates = O.literal_lm_forward(ref, torch.tensor(tok), rstates, L)
        rloss = O.nll_loss_literal(rscores, torch.tensor(tgt))
        rloss.backward()
        rstates = [(h.detach(), c.detach()) for h, c in rstates]
        assert_out(scores.detach().cpu().numpy(), rscores.detach().numpy(), f"scores{i}")
        assert abs(loss.item() - rloss.item()) < 1e-4 * abs(rloss.item())
        for k, p in model.named_parameters():
            assert_grad(p.grad.cpu().numpy(), ref[k].grad.numpy(), f"G{i}.{k}")
        norm = optim.clip_sgd_step(model.parameters(), lr=1.0, max_norm=0.25)
        with torch.no_grad():
            rnorm = torch.nn.utils.clip_grad_norm_(list(ref.values()), 0.25)
            for p in ref.values():
                p -= 1.0 * p.grad
        assert abs(float(norm) - float(rnorm)) < 1e-4 * float(rnorm)
    for k, v in model.state_dict().items():
        assert_out(v.cpu().numpy(), ref[k].detach().numpy(), "final." + k, atol=2e-5, rtol=1e-3)


def test_reference_lm_network_with_dropout_is_finite_and_reproducible():
    from vmlmf_amd import nll_loss
    outs = []
    for _ in range(2):
        model = _lm_model(0.5, seed=3).to(DEV)
        model.train()
        torch.manual_seed(17)
        rng = np.random.Generator(np.random.PCG64(5))
        tok = torch.tensor(rng.integers(0, 10000, size=(35, 20)), device=DEV)
        tgt = torch.tensor(rng.integers(0, 10000, size=(35, 20)), device=DEV)
        scores, _ = model(tok, model.state_init(20))
        loss = nll_loss(scores, tgt)
        loss.backward()
        assert np.isfinite(loss.item())
        grads = {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters()}
        assert all(np.all(np.isfinite(g)) for g in grads.values())
        outs.append((scores.detach().cpu().numpy(), grads))
    assert np.array_equal(outs[0][0], outs[1][0])
    for k in outs[0][1]:
        assert np.array_equal(outs[0][1][k], outs[1][1][k]), k


# ---- the HAR network and stacks -------------------------------------------------------------------------------------------------
def test_opp_net_three_adam_steps_vs_literal():
    """Net(77, [180], w_rank=64, u_rank=[64], cell=MyVMLMFCell) through train.py's loop (cross-entropy, Adam), three steps, against
    the literal harness with torch's Adam on host fp64 copies."""
    from vmlmf_amd import Net, MyVMLMFCell
    torch.manual_seed(4)
    net = Net(77, [180], w_rank=64, u_rank=[64], cell=MyVMLMFCell)
    ref_net = {k: v.detach().double().clone().requires_grad_(True) for k, v in net.named_parameters()}
    net = net.to(DEV)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    ropt = torch.optim.Adam(list(ref_net.values()), lr=1e-3)
    x, tgt = O.synthetic_batch(16, 24, 77, seed=99, classes=18)
    pfx = [k for k in ref_net if k.endswith("u_x")][0][: -len("u_x")]
    lin = [k for k in ref_net if k.endswith("weight")][0][: -len("weight")]
    for step in range(3):
        opt.zero_grad()
        logits = net(torch.tensor(x, device=DEV))
        loss = torch.nn.functional.cross_entropy(logits, torch.tensor(tgt, device=DEV))
        loss.backward()
        opt.step()
        ropt.zero_grad()
        P = {k[len(pfx):]: v for k, v in ref_net.items() if k.startswith(pfx)}
        rloss, rlogits = O.literal_train_step_har(P, ref_net[lin + "weight"], ref_net[lin + "bias"], torch.tensor(x, dtype=torch.float64),
                                                  torch.tensor(tgt))
        rloss.backward()
        ropt.step()
        assert_out(logits.detach().cpu().numpy(), rlogits.detach().numpy(), f"logits{step}")
        assert abs(loss.item() - rloss.item()) < 1e-4 * abs(rloss.item()) + 1e-6
    for k, p in net.named_parameters():
        assert_out(p.detach().cpu().numpy(), ref_net[k].detach().numpy(), "final." + k, atol=2e-5, rtol=1e-3)


def test_two_layer_wide_mylstm_vs_oracle():
    """MyLSTM of two wide layers: vmlmf_stack_query refuses the stack, the module chains the layers."""
    from vmlmf_amd import MyLSTM, MyVMLMFCell
    torch.manual_seed(8)
    rnn = MyLSTM(64, hidden_layer_sizes=[128, 128], batch_first=True, w_rank=48, u_ranks=[56], cell=MyVMLMFCell)
    Ps = []
    for l in range(2):
        P = {k.split(".", 2)[2]: v.detach().double().clone().requires_grad_(True) for k, v in rnn.named_parameters()
             if k.startswith(f"rnncells.{l}.")}
        Ps.append(P)
    rnn = rnn.to(DEV)
    rng = np.random.Generator(np.random.PCG64(81))
    x = rng.standard_normal((6, 9, 64)).astype(np.float32)
    dy = rng.standard_normal((6, 9, 128)).astype(np.float32)
    xt = torch.tensor(x, device=DEV, requires_grad=True)
    y, _ = rnn(xt)
    (y * torch.tensor(dy, device=DEV)).sum().backward()
    xr = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    h = xr
    for P in Ps:
        h, _, _ = O.literal_sequence(O.V1, P, h, time_major=False)
    (h * torch.tensor(dy, dtype=torch.float64)).sum().backward()
    assert_out(y.detach().cpu().numpy(), h.detach().numpy(), "y")
    assert_grad(xt.grad.cpu().numpy(), xr.grad.numpy(), "dx")
    for l, P in enumerate(Ps):
        for k, v in P.items():
            assert_grad(dict(rnn.named_parameters())[f"rnncells.{l}.{k}"].grad.cpu().numpy(), v.grad.numpy(), f"L{l}.{k}")
