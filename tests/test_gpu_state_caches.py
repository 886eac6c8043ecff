"""GPU: host-side state kept between calls - Net's per-call plan, vmlmf_amd.optim.Adam's flat moment buffers and remembered
argument blocks, GraphedTrainStep's captured graph - against twins that never kept anything, after the module or the optimizer
changed between calls.  Twins on the same kernels must agree bit for bit (the kernels are deterministic); the fp64 oracle and
torch.optim.Adam within the suite's tolerances.  The optimizer cases check on the host, before any launch, that the next step
reads and writes the buffers the optimizer's state points at."""
import copy
import io
import pickle

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import vmlmf_amd
import vmlmf_oracle as O
from hip_util import assert_grad, assert_out
from vmlmf_amd import MyLSTM, MyVMLMFCell, Net, _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
I, B, T = 9, 16, 12
CONFIGS = [(40, 8), (180, 16)]          # (hidden, rank): the headline family Net._fast takes


def _net(H, r, seed=0):
    torch.manual_seed(seed)
    return Net(I, layer_sizes=[H], w_rank=r, u_rank=[r], model=MyLSTM, cell=MyVMLMFCell).to(DEV)


def _batch(classes=18, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, I, generator=g).to(DEV)
    t = torch.randint(0, classes, (B,), generator=g).to(DEV)
    dz = torch.randn(B, classes, generator=g).to(DEV)
    return x, t, dz


def _twin(net):
    """A new Net of net's current structure, loaded from its state_dict(): it has never run, so it has no plan."""
    cells = list(net.rnn.rnncells)
    c0 = cells[0]
    torch.manual_seed(123)
    twin = Net(I, layer_sizes=[c.hidden_size for c in cells], w_rank=c0.w_rank, u_rank=[c0.u_ranks], model=MyLSTM,
               cell=MyVMLMFCell)
    twin.lin = nn.Linear(net.lin.in_features, net.lin.out_features)
    twin.load_state_dict(net.state_dict())
    return twin.to(DEV)


def _run(net, x, t, dz, how):
    """One forward (net(x) with a fixed upstream gradient, or net.loss) + backward: (output, {name: gradient or None})."""
    net.zero_grad(set_to_none=True)
    if how == "forward":
        out = net(x)
        (out * dz).sum().backward()
    else:
        out = net.loss(x, t)
        out.backward()
    return out.detach().clone(), {k: None if p.grad is None else p.grad.clone() for k, p in net.named_parameters()}


def _oracle(net, x, t, dz, how):
    """fp64: the literal recurrence of every layer (vmlmf_oracle), F.linear, cross-entropy; autograd for the gradients."""
    P = [O.to_torch({k: p.detach().cpu().numpy() for k, p in c.named_parameters()}, dtype=torch.float64, requires_grad=True)
         for c in net.rnn.rnncells]
    W = net.lin.weight.detach().double().cpu().requires_grad_(True)
    b = net.lin.bias.detach().double().cpu().requires_grad_(True)
    h = torch.tensor(x.cpu().numpy(), dtype=torch.float64)
    for Pl in P:
        h, hT, _ = O.literal_sequence(O.V1, Pl, h, None, None, time_major=False)
    z = F.linear(hT, W, b)
    if how == "forward":
        out = z
        (z * dz.double().cpu()).sum().backward()
    else:
        out = F.cross_entropy(z, t.cpu())
        out.backward()
    grads = {f"rnn.rnncells.{l}.{k}": v.grad for l, Pl in enumerate(P) for k, v in Pl.items()}
    grads.update({"lin.weight": W.grad, "lin.bias": b.grad})
    return out.detach(), grads


def _check_against_twin_and_oracle(net, x, t, dz):
    twin = _twin(net)
    for how in ("forward", "loss"):
        got, g_got = _run(net, x, t, dz, how)
        want, g_want = _run(twin, x, t, dz, how)
        assert got.shape == want.shape, (how, got.shape, want.shape)
        assert torch.equal(got, want), how
        assert g_got.keys() == g_want.keys()
        for k in g_got:
            assert (g_got[k] is None) == (g_want[k] is None), (how, k)
            assert g_got[k] is None or torch.equal(g_got[k], g_want[k]), (how, k)
        ref, g_ref = _oracle(net, x, t, dz, how)
        assert_out(got.cpu().numpy(), ref.numpy(), f"{how}.out")
        for k, gr in g_ref.items():
            assert_grad(g_got[k].cpu().numpy(), gr.numpy(), f"{how}.{k}")
        assert all(p.grad is None for p in net.cell.parameters())          # the reference's unused cell


def _warm(net, x, t, dz):
    """Calls before the change: both entry points build and use the per-call plan."""
    for how in ("forward", "loss"):
        _run(net, x, t, dz, how)


# ---- Net's per-call plan ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,r", CONFIGS)
def test_net_follows_a_new_classifier_of_the_same_size(H, r):
    net = _net(H, r)
    x, t, dz = _batch()
    _warm(net, x, t, dz)
    torch.manual_seed(7)
    net.lin = nn.Linear(H, 18).to(DEV)
    _check_against_twin_and_oracle(net, x, t, dz)


@pytest.mark.parametrize("H,r", CONFIGS)
def test_net_follows_a_new_classifier_with_more_classes_than_the_epilogue_carries(H, r):
    net = _net(H, r)
    x, t, dz = _batch()
    _warm(net, x, t, dz)
    C = 40
    assert C > _lib.HEAD_MAX_CLASSES
    torch.manual_seed(7)
    net.lin = nn.Linear(H, C).to(DEV)
    x, t, dz = _batch(classes=C, seed=2)
    _check_against_twin_and_oracle(net, x, t, dz)
    assert net(x).shape == (B, C)


@pytest.mark.parametrize("H,r", CONFIGS)
def test_net_follows_a_classifier_weight_assigned_anew(H, r):
    """A new Parameter in the existing Linear: more classes than the epilogue carries, through the same parameter dict."""
    net = _net(H, r)
    x, t, dz = _batch()
    _warm(net, x, t, dz)
    g = torch.Generator().manual_seed(8)
    net.lin.weight = nn.Parameter((0.1 * torch.randn(40, H, generator=g)).to(DEV))
    net.lin.bias = nn.Parameter((0.1 * torch.randn(40, generator=g)).to(DEV))
    net.lin.out_features = 40
    x, t, dz = _batch(classes=40, seed=2)
    _check_against_twin_and_oracle(net, x, t, dz)


@pytest.mark.parametrize("H,r", CONFIGS)
def test_net_follows_a_new_recurrent_cell(H, r):
    net = _net(H, r)
    x, t, dz = _batch()
    _warm(net, x, t, dz)
    torch.manual_seed(9)
    net.rnn.rnncells[0] = MyVMLMFCell(I, H, w_rank=r, u_ranks=r).to(DEV)
    _check_against_twin_and_oracle(net, x, t, dz)


@pytest.mark.parametrize("H,r", CONFIGS)
def test_net_follows_a_new_two_layer_stack(H, r):
    net = _net(H, r)
    x, t, dz = _batch()
    _warm(net, x, t, dz)
    torch.manual_seed(10)
    net.rnn = MyLSTM(I, hidden_layer_sizes=[H, H], batch_first=True, w_rank=r, u_ranks=[r], cell=MyVMLMFCell).to(DEV)
    _check_against_twin_and_oracle(net, x, t, dz)


@pytest.mark.parametrize("H,r", CONFIGS)
def test_net_follows_a_recurrent_parameter_assigned_anew(H, r):
    net = _net(H, r)
    x, t, dz = _batch()
    _warm(net, x, t, dz)
    cell = net.rnn.rnncells[0]
    g = torch.Generator().manual_seed(11)
    cell.u_h = nn.Parameter((0.1 * torch.randn(H, r, generator=g)).to(DEV))
    _check_against_twin_and_oracle(net, x, t, dz)


def _train(net, x, t, steps=3):
    opt = vmlmf_amd.optim.Adam(net.parameters(), lr=2e-3)
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        net.loss(x, t).backward()
        opt.step()
    return opt


def _pickled(net):
    return pickle.loads(pickle.dumps(net))


def _saved(net):
    buf = io.BytesIO()
    torch.save(net, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=False)


@pytest.mark.parametrize("H,r", CONFIGS)
@pytest.mark.parametrize("how", [_pickled, _saved, copy.deepcopy], ids=["pickle", "torch_save", "deepcopy"])
def test_a_trained_net_copies_with_its_own_plan(H, r, how):
    """pickle / torch.save + torch.load / copy.deepcopy after training: the copy computes what the original does, and after an
    in-place change to the copy's parameters it follows them while the original stays as it was."""
    net = _net(H, r)
    x, t, dz = _batch()
    _train(net, x, t)
    before = {h: _run(net, x, t, dz, h) for h in ("forward", "loss")}
    c = how(net)
    assert "_fast_plan" not in c.__dict__
    for h in ("forward", "loss"):
        got, g = _run(c, x, t, dz, h)
        assert torch.equal(got, before[h][0]), h
        for k, v in g.items():
            assert (v is None) == (before[h][1][k] is None) and (v is None or torch.equal(v, before[h][1][k])), (h, k)
    with torch.no_grad():
        for p in c.parameters():
            p.mul_(1.25)
    _check_against_twin_and_oracle(c, x, t, dz)
    for h in ("forward", "loss"):
        got, _ = _run(net, x, t, dz, h)
        assert torch.equal(got, before[h][0]), h
        assert not torch.equal(_run(c, x, t, dz, h)[0], got), h


# ---- vmlmf_amd.optim.Adam: flat buffers and remembered argument blocks ------------------------------------------------------
SHAPES = [(9, 16), (720, 16), (1, 180), (720,), (18, 180), (18,)]


def _params(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    mine = [nn.Parameter(torch.randn(*s, generator=g).to(DEV)) for s in shapes]
    return mine, [nn.Parameter(p.detach().clone()) for p in mine], g


def _feed(g, *sides, in_place=False):
    """The same fresh gradients on every side: assigned (after zero_grad(set_to_none=True)) or copied into the tensors that
    zero_grad(set_to_none=False) left."""
    for ps in zip(*sides):
        gr = torch.randn(*ps[0].shape, generator=g).to(DEV)
        for p in ps:
            if in_place and p.grad is not None:
                p.grad.copy_(gr)
            else:
                p.grad = gr.clone()


def _close(mine, ref):
    for a, b in zip(mine, ref):
        a, b = a.detach(), b.detach()
        assert float((a - b).abs().max()) <= 2e-6 * max(1.0, float(b.abs().max()))


def _next_step_is_live(opt):
    """Host side, no launch: every pointer the remembered argument blocks of the next step() hold for a parameter's moments and
    step count is the address of that parameter's state in opt.state (nothing remembered: the step builds its blocks anew)."""
    cached = opt.__dict__.get("_step_cache")
    if cached is None:
        return True
    by_ptr = {p.data_ptr(): p for group in opt.param_groups for p in group["params"]}
    for (args, _live), tl in zip(cached[1], cached[2]):
        m, v, steps = args[1], args[2], args[3]
        for i in range(tl.count):
            st = opt.state.get(by_ptr[tl.param[i]], {})
            if not all(k in st for k in ("exp_avg", "exp_avg_sq", "step")):
                return False
            if (st["exp_avg"].data_ptr() != m + 4 * tl.state_offset[i] or st["exp_avg_sq"].data_ptr() != v + 4 * tl.state_offset[i]
                    or st["step"].data_ptr() != steps + 4 * tl.step_index[i]):
                return False
    return True


def _stepped(shapes, seed, steps=3):
    mine, ref, g = _params(shapes, seed)
    o1, o2 = vmlmf_amd.optim.Adam(mine, lr=2e-3), torch.optim.Adam(ref, lr=2e-3)
    for _ in range(steps):
        _feed(g, mine, ref)
        o1.step(), o2.step()
    return mine, ref, g, o1, o2


# (more than MAX_TENSORS parameters: a step takes two tensor lists)
TWO_LISTS = [(3, 5 + k % 7) for k in range(_lib.MAX_TENSORS + 5)]


@pytest.mark.parametrize("shapes", [SHAPES, TWO_LISTS], ids=["six", "two_tensor_lists"])
def test_adam_reset_to_an_empty_state_restarts_at_step_one(shapes):
    """load_state_dict(<a fresh optimizer's state_dict()>) into an optimizer that has stepped: like torch.optim.Adam, and bit for
    bit like a new vmlmf_amd.optim.Adam on the same parameters, the next step is step 1 again."""
    mine, ref, g, o1, o2 = _stepped(shapes, seed=3)
    o1.load_state_dict(vmlmf_amd.optim.Adam(mine, lr=2e-3).state_dict())
    o2.load_state_dict(torch.optim.Adam(ref, lr=2e-3).state_dict())
    assert _next_step_is_live(o1)
    twin = [nn.Parameter(p.detach().clone()) for p in mine]
    o3 = vmlmf_amd.optim.Adam(twin, lr=2e-3)
    for _ in range(3):
        _feed(g, mine, ref, twin)
        o1.step(), o2.step(), o3.step()
    _close(mine, ref)
    for a, c in zip(mine, twin):
        assert torch.equal(a, c)
        assert torch.equal(o1.state[a]["exp_avg"], o3.state[c]["exp_avg"])
        assert torch.equal(o1.state[a]["exp_avg_sq"], o3.state[c]["exp_avg_sq"])
        assert float(o1.state[a]["step"]) == 3.0


@pytest.mark.parametrize("source", ["own", "torch"])
@pytest.mark.parametrize("shapes", [SHAPES, TWO_LISTS], ids=["six", "two_tensor_lists"])
def test_adam_resumes_a_checkpoint_in_an_optimizer_that_has_stepped(source, shapes):
    """A checkpoint taken after 3 steps, 2 more steps, the checkpoint loaded, 3 more: like torch.optim.Adam resumed the same way,
    and bit for bit like a new vmlmf_amd.optim.Adam resumed from it."""
    mine, ref, g, o1, o2 = _stepped(shapes, seed=4)
    ck = copy.deepcopy((o1 if source == "own" else o2).state_dict())
    ck_ref = copy.deepcopy(o2.state_dict())
    for _ in range(2):
        _feed(g, mine, ref)
        o1.step(), o2.step()
    o1.load_state_dict(ck)
    o2.load_state_dict(ck_ref)
    assert _next_step_is_live(o1)
    twin = [nn.Parameter(p.detach().clone()) for p in mine]
    o3 = vmlmf_amd.optim.Adam(twin, lr=2e-3)
    o3.load_state_dict(ck)
    for _ in range(3):
        _feed(g, mine, ref, twin)
        o1.step(), o2.step(), o3.step()
        assert _next_step_is_live(o1)
    _close(mine, ref)
    for a, c in zip(mine, twin):
        assert torch.equal(a, c)
    assert float(o1.state[mine[0]]["step"]) == 6.0


@pytest.mark.parametrize("shapes", [SHAPES, TWO_LISTS], ids=["six", "two_tensor_lists"])
def test_adam_follows_lr_changes_new_groups_and_zero_grad_modes(shapes):
    """Between steps: the learning rate changed in param_groups, a parameter group added, gradients zeroed in place
    (zero_grad(set_to_none=False): same addresses, remembered argument blocks) or dropped (set_to_none=True: new ones)."""
    mine, ref, g, o1, o2 = _stepped(shapes, seed=5, steps=2)
    extra_m, extra_r, _ = _params([(7, 11), (33,)], seed=6)
    for it in range(6):
        if it == 1:
            for o in (o1, o2):
                o.param_groups[0]["lr"] = 5e-4
        if it == 2:
            o1.add_param_group(dict(params=extra_m, lr=1e-3, weight_decay=0.01))
            o2.add_param_group(dict(params=extra_r, lr=1e-3, weight_decay=0.01))
        if it == 4:
            for o in (o1, o2):
                o.param_groups[1]["lr"] = 3e-3
        in_place = it % 2 == 1
        for o in (o1, o2):
            o.zero_grad(set_to_none=not in_place)
        sides_m = mine + (extra_m if it >= 2 else [])
        sides_r = ref + (extra_r if it >= 2 else [])
        _feed(g, sides_m, sides_r, in_place=in_place)
        assert _next_step_is_live(o1)
        o1.step(), o2.step()
    _close(mine + extra_m, ref + extra_r)
    assert float(o1.state[mine[0]]["step"]) == 8.0 and float(o1.state[extra_m[0]]["step"]) == 4.0


# ---- GraphedTrainStep ------------------------------------------------------------------------------------------------------
def _graphed_pair(H=40, r=8, n=8):
    """A GraphedTrainStep and its eager twin (same model values, vmlmf_amd.optim.Adam, the step's own body), and n batches."""
    a = _net(H, r, seed=1)
    b = _twin(a)
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(B, T, I, generator=g).to(DEV) for _ in range(n)]
    ts = [torch.randint(0, 18, (B,), generator=g).to(DEV) for _ in range(n)]
    step = vmlmf_amd.GraphedTrainStep(a, vmlmf_amd.cross_entropy, vmlmf_amd.optim.Adam(a.parameters(), lr=2e-3), xs[0], ts[0],
                                      warmup=2)
    opt = vmlmf_amd.optim.Adam(b.parameters(), lr=2e-3)
    recorded = {id(p): (st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"].data_ptr())
                for p, st in step.optimizer.state.items()}
    return a, b, step, opt, xs, ts, recorded


def _eager_step(b, opt, x, t):
    opt.zero_grad(set_to_none=True)
    loss = b.loss(x, t)
    loss.backward(vmlmf_amd.unit_gradient(x.device))
    opt.step()
    return loss.detach()


def _graph_reads_the_state(step, recorded):
    """Host side, no launch: the moments and step counts the captured graph updates are still the optimizer's state."""
    st = step.optimizer.state
    return all(p in st and (st[p]["exp_avg"].data_ptr(), st[p]["exp_avg_sq"].data_ptr(), st[p]["step"].data_ptr()) == recorded[id(p)]
               for p in step.optimizer.param_groups[0]["params"] if id(p) in recorded)


def _graphed_run(event):
    a, b, step, opt, xs, ts, recorded = _graphed_pair()
    ck = ck_model = None
    for it, (x, t) in enumerate(zip(xs, ts)):
        if it == 2:
            ck = copy.deepcopy(step.optimizer.state_dict())
            ck_model = copy.deepcopy(a.state_dict())
        if it == 5:
            if event == "optimizer_checkpoint":
                step.optimizer.load_state_dict(ck)
                opt.load_state_dict(ck)
            elif event == "empty_state":
                step.optimizer.load_state_dict(vmlmf_amd.optim.Adam(a.parameters(), lr=2e-3).state_dict())
                opt.load_state_dict(vmlmf_amd.optim.Adam(b.parameters(), lr=2e-3).state_dict())
            elif event == "model_state":
                a.load_state_dict(ck_model)
                b.load_state_dict(ck_model)
            assert _graph_reads_the_state(step, recorded)
        la = step(x, t).clone()
        lb = _eager_step(b, opt, x, t)
        assert abs(float(la) - float(lb)) <= 1e-6 * max(1.0, abs(float(lb))), (event, it)
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.allclose(pa, pb, rtol=1e-5, atol=1e-7), event
    for pa, pb in zip(a.parameters(), b.parameters()):
        sa, sb = step.optimizer.state[pa], opt.state[pb]
        assert float(sa["step"]) == float(sb["step"]), event
        assert torch.allclose(sa["exp_avg"], sb["exp_avg"], rtol=1e-4, atol=1e-9), event
    return step


def test_graphed_step_resumes_an_optimizer_checkpoint_between_replays():
    step = _graphed_run("optimizer_checkpoint")
    # resumed at the checkpoint's count (2) + the replays after the load (3)
    assert float(step.optimizer.state[next(step.model.rnn.parameters())]["step"]) == 5.0


def test_graphed_step_restarts_after_an_empty_optimizer_state_is_loaded():
    step = _graphed_run("empty_state")
    assert float(step.optimizer.state[next(step.model.rnn.parameters())]["step"]) == 3.0


def test_graphed_step_follows_model_load_state_dict_between_replays():
    step = _graphed_run("model_state")
    assert float(step.optimizer.state[next(step.model.rnn.parameters())]["step"]) == 8.0


def test_graphed_step_refuses_a_parameter_group_added_after_the_capture():
    a, b, step, opt, xs, ts, _ = _graphed_pair(n=2)
    step(xs[0], ts[0])
    step.optimizer.add_param_group(dict(params=[nn.Parameter(torch.zeros(4, device=DEV))]))
    with pytest.raises(RuntimeError, match="parameter group"):
        step(xs[1], ts[1])
