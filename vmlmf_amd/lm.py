"""Drop-in counterparts of the reference's language-model layers, backed by the HIP kernels.

  MyVMLSTM       V/src/models/vmlmf_lm.py:178-280   forward(x:(T,B,X), (h,c)) -> (y, (h,c))
  MyVMLSTMGroup  V/src/models/vmlmf_lm.py:53-174    (the reference only runs at batch 40: its scratch is
                                                     hard-coded, 112-113; this implementation has no limit)
  Embed, Linear, Model   V/src/models/vmlmf_lm.py:33-51, 345-364, 366-440: the rest of the LM network around those layers
                         (SURVEY section 8f rank 3).  Embedding lookup and the vocabulary projection (one library GEMM) are
                         stock ops; the loss that consumes the scores is vmlmf_amd.nll_loss (fused kernels).  The reference's
                         dense "custom" LSTM layer (283-339) is the uncompressed baseline, off the VMLMF path: class LSTM
                         below keeps it available in stock library ops (Model(lstm_type="custom")); dense_layer= overrides it.
Parameter names, shapes and registration order follow the reference (state_dict compatible).
"""
from __future__ import annotations

import torch
from torch import nn

from . import _lib
from .functional import vmlmf_sequence


class MyVMLSTM(nn.Module):
    variant = _lib.V3_LM

    def __init__(self, input_size, hidden_size, dropout=0, w_rank=None, u_ranks=None):
        super().__init__()
        self.input_size = input_size
        self.hidden_size = hidden_size
        self.dropout = dropout
        self.w_rank = w_rank
        self.u_ranks = u_ranks
        # the reference allocates uninitialised storage and lets Model.reset_parameters fill it
        # (vmlmf_lm.py:407-410); zeros here: no RNG draw, so a seeded Model init stays in step
        self.u_x = nn.Parameter(torch.zeros(input_size, w_rank))
        self.u_h = nn.Parameter(torch.zeros(hidden_size, u_ranks))
        self.w_x = nn.Parameter(torch.zeros(4 * hidden_size, w_rank))
        self.w_h = nn.Parameter(torch.zeros(4 * hidden_size, u_ranks))
        self.b_x = nn.Parameter(torch.zeros(4 * hidden_size))
        self.b_h = nn.Parameter(torch.zeros(4 * hidden_size))
        self.dia_x = nn.Parameter(torch.zeros(1, input_size))
        self.dia_h = nn.Parameter(torch.zeros(1, hidden_size))
        self.cnt = 0

    def __repr__(self):
        return f"LSTM(input: {self.input_size}, hidden: {self.hidden_size})"

    def kernel_params(self):
        return (self.dia_x, self.dia_h, self.u_x, self.w_x, self.b_x, self.b_h, self.u_h, self.w_h)

    def _run(self, x, h, c, drop=None):
        return vmlmf_sequence(self.variant, x, h, c, self.kernel_params(), self.w_rank, [self.u_ranks],
                              g=1, time_major=True, dtype=getattr(self, "compute_dtype", "f32"), pack_cache=getattr(self, "_pack_cache", None),
                              drop=drop)

    def lstm_step(self, x, h, c):
        """One timestep (vmlmf_lm.py:222-269): T = 1 of the sequence kernels."""
        _, hn, cn = self._run(x.unsqueeze(0), h, c)
        return hn, cn

    def forward(self, x, states, drop=None):
        """drop = (p, snapshot, site), or (p, snapshot, site, True) for the locked form (one (B, H) mask for every time step:
        docs/design/lm_locked.md): the returned y went through Model's dropout (vmlmf_lm.py:438-439) - inside this layer's own
        launches where the library covers it (functional.vmlmf_sequence)."""
        h, c = states
        y, hT, cT = self._run(x, h, c, drop)
        return y, (hT, cT)


class MyVMLSTMGroup(nn.Module):
    variant = _lib.V4_LM_GROUP

    def __init__(self, input_size, hidden_size, dropout=0, w_rank=None, u_ranks=None, g=2):
        super().__init__()
        self.input_size = input_size
        self.hidden_size = hidden_size
        self.dropout = dropout
        self.g = g
        self.w_rank = w_rank
        self.u_ranks = u_ranks
        self.u_x = nn.Parameter(torch.zeros(input_size, w_rank))
        self.w_x = nn.Parameter(torch.zeros(4 * hidden_size, w_rank))
        self.u_h = nn.ParameterList([nn.Parameter(torch.zeros(g, int(hidden_size / g), u_ranks[s]))
                                     for s in range(self.g)])
        self.v_h = nn.ParameterList([nn.Parameter(torch.zeros(g, u_ranks[s], 4 * int(hidden_size / g)))
                                     for s in range(self.g)])
        self.b_x = nn.Parameter(torch.zeros(4 * hidden_size))
        self.b_h = nn.Parameter(torch.zeros(4 * hidden_size))
        self.dia_x = nn.Parameter(torch.zeros(1, input_size))
        self.dia_h = nn.Parameter(torch.zeros(1, hidden_size))
        self.cnt = 0

    def __repr__(self):
        return f"LSTM(input: {self.input_size}, hidden: {self.hidden_size})"

    def kernel_params(self):
        out = [self.dia_x, self.dia_h, self.u_x, self.w_x, self.b_x, self.b_h]
        for s in range(self.g):
            out += [self.u_h[s], self.v_h[s]]
        return tuple(out)

    def _run(self, x, h, c, drop=None):
        return vmlmf_sequence(self.variant, x, h, c, self.kernel_params(), self.w_rank, list(self.u_ranks),
                              g=self.g, time_major=True, dtype=getattr(self, "compute_dtype", "f32"), pack_cache=getattr(self, "_pack_cache", None),
                              drop=drop)

    def lstm_step(self, x, h, c):
        _, hn, cn = self._run(x.unsqueeze(0), h, c)
        return hn, cn

    def forward(self, x, states, drop=None):
        """drop = (p, snapshot, site), or (p, snapshot, site, True) for the locked form (one (B, H) mask for every time step:
        docs/design/lm_locked.md): the returned y went through Model's dropout (vmlmf_lm.py:438-439) - inside this layer's own
        launches where the library covers it (functional.vmlmf_sequence)."""
        h, c = states
        y, hT, cT = self._run(x, h, c, drop)
        return y, (hT, cT)


class LSTM(nn.Module):
    """The reference's dense "custom" layer (vmlmf_lm.py:283-339): the uncompressed baseline Model(lstm_type="custom")
    builds.  Not part of the VMLMF path, so stock library ops on whatever device the tensors live on: the input side of all
    T steps is one GEMM ahead of the time loop, the recurrence one addmm per step.  Same parameter names and shapes."""

    def __init__(self, input_size, hidden_size, dropout=0):
        super().__init__()
        self.input_size, self.hidden_size, self.dropout = input_size, hidden_size, dropout
        self.w_x = nn.Parameter(torch.zeros(4 * hidden_size, input_size))
        self.w_h = nn.Parameter(torch.zeros(4 * hidden_size, hidden_size))
        self.b_x = nn.Parameter(torch.zeros(4 * hidden_size))
        self.b_h = nn.Parameter(torch.zeros(4 * hidden_size))

    def __repr__(self):
        return f"LSTM(input: {self.input_size}, hidden: {self.hidden_size})"

    def forward(self, x, states):
        h, c = states
        T, B, _ = x.shape
        H = self.hidden_size
        gx = torch.addmm(self.b_x + self.b_h, x.reshape(T * B, -1), self.w_x.t()).view(T, B, 4 * H)
        w_ht = self.w_h.t()
        ys = []
        for t in range(T):
            i, f, o, n = torch.addmm(gx[t], h, w_ht).split(H, 1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(n)
            h = torch.sigmoid(o) * torch.tanh(c)
            ys.append(h)
        return torch.stack(ys), (h, c)


class Embed(nn.Module):
    """Embedding table indexed by token id (vmlmf_lm.py:33-51)."""

    def __init__(self, vocab_size, embed_size):
        super().__init__()
        self.vocab_size = vocab_size
        self.embed_size = embed_size
        self.w = nn.Parameter(torch.zeros(vocab_size, embed_size))

    def forward(self, x):
        from .functional import embedding
        return embedding(self.w, x)      # the gather is the stock op; the table's gradient is the package's kernel on HIP tensors

    def __repr__(self):
        return f"Embedding(vocab: {self.vocab_size}, embedding: {self.embed_size})"


class Linear(nn.Module):
    """Vocabulary projection (vmlmf_lm.py:345-364): (T, B, H) -> (T*B, V) scores, one library GEMM."""

    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.input_size = input_size
        self.hidden_size = hidden_size
        self.w = nn.Parameter(torch.zeros(hidden_size, input_size))
        self.b = nn.Parameter(torch.zeros(hidden_size))

    def forward(self, x):
        return torch.addmm(self.b, x.view(-1, x.size(2)), self.w.t())

    def __repr__(self):
        return f"FC(input: {self.input_size}, output: {self.hidden_size})"


def stack_layers(rnns, x, states, drops=None):
    """The layer loop of Model.forward (vmlmf_lm.py:437-439: `x, states[i] = rnn(x, states[i]); x = dropout(x)`) as ONE launch per
    direction with the carried states as initial states (functional.vmlmf_stack): the wavefront kernels for hidden sizes up to 256
    (MyVMLSTM layers, no dropout between the layers), or - layers of the PTB size, MyVMLSTM or MyVMLSTMGroup, at batch sizes whose
    clusters are co-resident for all layers (up to 128 rows for two layers: what a GPU of an 8-GPU node holds of configs[4]) - the
    clustered form (csrc/vmlmf_rbx.hip), which also applies the dropout behind every layer inside its launches (drops: one
    (p, snapshot, site) per layer - (p, snapshot, site, True): the locked form; None: no dropout behind that layer -; the returned
    activations are then the top layer's dropped copy).
    Returns (y, [(hT, cT) per layer]), or None when the stack is not covered: the caller loops over the layers."""
    rnns = list(rnns)
    if not x.is_cuda or len(rnns) < 2:
        return None
    kind = type(rnns[0])
    if kind not in (MyVMLSTM, MyVMLSTMGroup) or not all(type(r) is kind for r in rnns):
        return None
    r0 = rnns[0]
    if any((r.input_size, r.hidden_size, r.w_rank, r.u_ranks) != (r0.input_size, r0.hidden_size, r0.w_rank, r0.u_ranks) for r in rnns):
        return None
    if any(getattr(r, "compute_dtype", "f32") != "f32" for r in rnns):
        return None
    from .functional import vmlmf_stack
    h0 = torch.stack([st[0] for st in states])
    c0 = torch.stack([st[1] for st in states])
    ur = r0.u_ranks if isinstance(r0.u_ranks, (list, tuple)) else [r0.u_ranks]
    out = vmlmf_stack(variant=r0.variant, x=x, layer_params=[r.kernel_params() for r in rnns], w_rank=r0.w_rank,
                      u_ranks=list(ur), g=getattr(r0, "g", 1), time_major=True, h0=h0, c0=c0, drops=drops)
    if out is None:
        return None
    y, hs, cs = out
    return y, [(hs[i], cs[i]) for i in range(len(rnns))]


class Model(nn.Module):
    """The language model of lm_test.py (vmlmf_lm.py:366-440): Embed -> dropout -> layer_num x (LSTM layer ->
    dropout) -> Linear.  Constructor logic is the reference's, quirks included: `u_ranks` is reduced to its last
    element unless lstm_type is the string "vm_group", while the group layers are only built for the string
    "vmgroup" -- so, as in the reference, "vmgroup" with a rank list fails in MyVMLSTMGroup's constructor and
    "vm_group" silently builds torch.nn.LSTM layers.  Build MyVMLSTMGroup layers directly for the group variant."""

    def __init__(self, vocab_size, hidden_size, layer_num, dropout, winit, w_rank=None, u_ranks=None,
                 lstm_type="pytorch", dense_layer=None, tie_weights=False, embed_dropout=0.0, locked_dropout=False, input_dropout=None,
                 hidden_dropout=None, output_dropout=None):
        """dense_layer: overrides the class built for lstm_type="custom" (default: LSTM above, the reference's dense baseline
        layer in stock ops); any class with the signature (input_size, hidden_size) and forward(x, states).
        tie_weights, embed_dropout: NOT part of the reference's interface - AWD-LSTM's --tied (tie_weights()) and --dropoute (the
        embed_dropout attribute); docs/design/lm_tied.md.
        locked_dropout, input_dropout, hidden_dropout, output_dropout: neither - AWD-LSTM's LockedDropout and its --dropouti,
        --dropouth and --dropout (the attributes of these names); docs/design/lm_locked.md."""
        super().__init__()
        self.embed_dropout = embed_dropout
        self.locked_dropout = locked_dropout
        self.input_dropout, self.hidden_dropout, self.output_dropout = input_dropout, hidden_dropout, output_dropout
        self.vocab_size = vocab_size
        self.hidden_size = hidden_size
        self.layer_num = layer_num
        self.winit = winit
        self.lstm_type = lstm_type
        self.embed = Embed(vocab_size, hidden_size)
        if u_ranks is not None and lstm_type != "vm_group":
            u_ranks = u_ranks[-1]
        if lstm_type == "vmgroup":
            rnns = [MyVMLSTMGroup(hidden_size, hidden_size, w_rank=w_rank, u_ranks=u_ranks) for _ in range(layer_num)]
        elif lstm_type == "custom":
            rnns = [(dense_layer or LSTM)(hidden_size, hidden_size) for _ in range(layer_num)]
        elif lstm_type != "vmlmf":
            rnns = [nn.LSTM(hidden_size, hidden_size) for _ in range(layer_num)]
        else:
            rnns = [MyVMLSTM(hidden_size, hidden_size, w_rank=w_rank, u_ranks=u_ranks) for _ in range(layer_num)]
        self.rnns = nn.ModuleList(rnns)
        self.fc = Linear(hidden_size, vocab_size)
        self.dropout = nn.Dropout(p=dropout)
        self.reset_parameters()
        if tie_weights:
            self.tie_weights()

    def reset_parameters(self):
        for param in self.parameters():          # (a tied table is met once: parameters() names a shared tensor once)
            nn.init.uniform_(param, -self.winit, self.winit)

    # ---- one table as embedding and vocabulary projection (weight tying); word-level embedding dropout: docs/design/lm_tied.md ----
    @property
    def tied(self):
        """True while fc.w IS embed.w (tie_weights())."""
        return self.fc.w is self.embed.w

    def tie_weights(self):
        """Weight tying (Press & Wolf; Inan et al.; AWD-LSTM's --tied): fc.w becomes the very Parameter embed.w is - embed.w's values
        are kept, as AWD-LSTM's `decoder.weight = encoder.weight` keeps them; Embed(V, H) and Linear(H, V) have the same (V, H) shape
        here.  parameters() then names the table once (one tensor and V H elements fewer: half of the PTB network, of every optimizer
        step and of the data-parallel gradient traffic); state_dict() keeps both keys, torch's behaviour, and the tie survives
        load_state_dict, .to() and copy.deepcopy.  loss(), distill_loss() and DynamicEval form the table's ONE gradient without a
        table-wide add: the embedding's backward adds its rows into the head's dW in place (functional.TiedGradient); forward()'s
        scores and every other use are correct through autograd's own accumulation.  Optimizers built before the call still
        hold the old fc.w: build them after it.  Returns self."""
        self.fc.w = self.embed.w
        return self

    def untie_weights(self):
        """fc.w gets a Parameter of its own again, a clone of the table.  Returns self."""
        if self.tied:
            w = self.embed.w
            self.fc.w = nn.Parameter(w.detach().clone(), requires_grad=w.requires_grad)
        return self

    @property
    def embed_dropout(self):
        """AWD-LSTM's embedding dropout (--dropoute), a probability in [0, 1): in training mode whole WORDS are dropped from the
        table for a forward pass - one factor per vocabulary row, 0 or 1 / (1 - embed_dropout), shared by every position that holds
        the word - in front of the element dropout of `dropout`.  On a HIP device inside the gather's and the table gradient's own
        launches (functional.embedding_dropout(word_p=)); on CPU tensors and under stock_dropout in stock ops
        (functional.embedding_dropout_stock).  ValueError for a bool or a value outside [0, 1)."""
        return getattr(self, "_embed_dropout", 0.0)

    @embed_dropout.setter
    def embed_dropout(self, value):
        from .functional import check_word_dropout
        check_word_dropout(value, "Model.embed_dropout")
        self._embed_dropout = float(value)

    # ---- locked (variational) dropout and a rate per site: docs/design/lm_locked.md ----
    @property
    def locked_dropout(self):
        """True: the three activation dropouts (behind the embedding, between the layers, behind the top layer) are AWD-LSTM's
        LockedDropout - ONE (B, H) mask per site and forward pass, shared by every time step - where nn.Dropout draws a factor for
        every (t, b, n).  On a HIP device inside the launches that apply the per-element dropout (no mask tensor, no added launch);
        on CPU tensors and under stock_dropout the rule in stock ops (functional.locked_dropout_stock).  ValueError unless a bool."""
        return getattr(self, "_locked_dropout", False)

    @locked_dropout.setter
    def locked_dropout(self, value):
        if not isinstance(value, bool):
            raise ValueError(f"vmlmf_amd: Model.locked_dropout must be a bool, got {value!r}")
        self._locked_dropout = value

    def _site_rate(name, doc):
        def get(self):
            return getattr(self, "_" + name, None)

        def put(self, value):
            if value is not None:
                from .functional import check_word_dropout
                check_word_dropout(value, "Model." + name)
                value = float(value)
            setattr(self, "_" + name, value)
        return property(get, put, doc=doc + "  A probability in [0, 1), or None: follow `dropout.p`.  ValueError for a bool or a "
                        "value outside [0, 1).")

    input_dropout = _site_rate("input_dropout", "The rate of dropout site 0, behind the embedding (AWD-LSTM's --dropouti).")
    hidden_dropout = _site_rate("hidden_dropout", "The rate of sites 1 .. L - 1, between the layers (AWD-LSTM's --dropouth).")
    output_dropout = _site_rate("output_dropout", "The rate of site L, behind the top layer (AWD-LSTM's --dropout).")
    del _site_rate

    def site_rates(self):
        """The drop probability of every site 0 .. L in the current mode (all zero in eval mode): input_dropout, hidden_dropout for
        each site between two layers, output_dropout; None among them reads `dropout.p`."""
        L, p = len(self.rnns), float(self.dropout.p)
        if not self.training:
            return [0.0] * (L + 1)
        pick = lambda v: p if v is None else v
        return [pick(self.input_dropout)] + [pick(self.hidden_dropout)] * (L - 1) + [pick(self.output_dropout)]

    def _site_dropout(self, x, p):
        """One site's dropout in stock ops (CPU tensors, stock_dropout): nn.Dropout - self.dropout itself at its own rate, so a
        model built without the new arguments runs the ops it ran - or AWD-LSTM's LockedDropout."""
        if self.locked_dropout:
            from .functional import locked_dropout_stock
            return locked_dropout_stock(x, p, self.training)
        if p == self.dropout.p or not self.training:
            return self.dropout(x)
        return torch.nn.functional.dropout(x, p, self.training)

    def _tied_gradient(self, x):
        """A fresh functional.TiedGradient for one loss call on tokens x where the table is tied and both ends take it, else None."""
        if not self.tied:
            return None
        if self.training and self.embed_dropout > 0 and getattr(self, "stock_dropout", False):
            return None                          # the word dropout in stock ops: autograd adds the two gradients up
        from .functional import tied_gradient
        return tied_gradient(self.embed.w, x)

    @classmethod
    def with_group_layers(cls, vocab_size, hidden_size, layer_num, dropout, winit, w_rank, u_ranks, g=2, tie_weights=False,
                          embed_dropout=0.0, locked_dropout=False, input_dropout=None, hidden_dropout=None, output_dropout=None):
        """The network of BASELINE configs[4] - Model with MyVMLSTMGroup layers - which the reference's constructor cannot build
        (lstm_type "vmgroup" reduces the rank list to its last element and MyVMLSTMGroup then fails, vmlmf_lm.py:387-392; "vm_group",
        the CLI's spelling, builds nn.LSTM).  NOT part of the reference's interface: the constructor above keeps the reference's
        behaviour, this puts the group layers in by hand (as a maintainer has to) and initialises every parameter as
        Model.reset_parameters does.  u_ranks: one rank per group rotation, e.g. [32, 32]."""
        model = cls(vocab_size, hidden_size, layer_num, dropout, winit, w_rank=w_rank, u_ranks=[list(u_ranks)[-1]], lstm_type="vmlmf",
                    locked_dropout=locked_dropout, input_dropout=input_dropout, hidden_dropout=hidden_dropout,
                    output_dropout=output_dropout)
        model.rnns = nn.ModuleList([MyVMLSTMGroup(hidden_size, hidden_size, w_rank=w_rank, u_ranks=list(u_ranks), g=g)
                                    for _ in range(layer_num)])
        model.lstm_type = "vmgroup"
        model.reset_parameters()
        model.embed_dropout = embed_dropout
        if tie_weights:
            model.tie_weights()
        return model

    def state_init(self, batch_size):
        dev = next(self.parameters()).device
        flat = self.lstm_type in ["custom", "vmlmf", "vmgroup", "hmd"]
        shape = (lambda layer: (batch_size, layer.hidden_size)) if flat else \
            (lambda layer: (1, batch_size, layer.hidden_size))
        return [(torch.zeros(*shape(layer), device=dev), torch.zeros(*shape(layer), device=dev)) for layer in self.rnns]

    def detach(self, states):
        return [(h.detach(), c.detach()) for (h, c) in states]

    def _stack(self, x, states, drops=None):
        """stack_layers() on this model's layers, unless dropout is active and not handed in (`drops`)."""
        if max(self.site_rates()) > 0 and drops is None:
            return None
        return stack_layers(self.rnns, x, states, drops)

    def forward(self, x, states):
        x, states = self.features(x, states)
        scores = self.fc(x)
        return scores, states

    def loss(self, x, y, states, *, lengths=None, label_smoothing=0.0, z_loss=0.0, unlikelihood=0.0, negatives=None, normalize="rows",
             return_parts=False, ar=0.0, tar=0.0):
        """nll_loss(self(x, states)[0], y) of the training loop (lm_test.py:200-202) without ever handing out the scores: the
        projection's output is overwritten by its own gradient inside the loss (functional.lm_head_loss), which is what the two
        backward GEMMs read.  Returns (loss, states); same values as the two-call form.  With every keyword at its default this is
        that call and nothing else.  The keywords add a trainer's other loss arguments as terms of the same pass
        (functional.lm_head_objective_loss; docs/design/lm_objective.md) - with z_r the scores of row r = t B + b, p = softmax(z_r):
            row_r = (1 - eps)(lse_r - z_r[y_r]) + eps (lse_r - mean z_r) + zeta lse_r^2 + alpha sum_{c in C_r} -log(max(1 - p_c, 1e-5))
            loss  = scale * sum over the valid rows of row_r
        lengths (B) integers, Model.score's contract: position (t, b) is valid iff t < lengths[b]; another row adds nothing and has
          no gradient.  Any other target outside [0, V) still makes the loss NaN.
        label_smoothing = eps in [0, 1) and z_loss = zeta >= 0: F.cross_entropy's smoothing and the squared log-partition penalty.
        unlikelihood = alpha >= 0: token-level unlikelihood training (Welleck et al.) against the candidate SET C_r of `negatives`
          (T, B, K) or (T B, K) int64, 1 <= K <= 256 - entries outside [0, V) (use -1) are padding, duplicates count once, the row's
          own target is ignored.  negatives=None: the paper's candidates, the input tokens x[0 .. t, b] of the minibatch
          (context_negatives(x)); given with alpha == 0 they are not read.
        normalize "rows": scale = B / (T B) as above, a mask only removes terms; "tokens": scale = B / max(valid positions, 1),
          formed on the device ("tokens" without lengths is "rows").
        return_parts=True: loss is (loss, nll, smooth, z, unlikelihood), the parts detached, scaled like the loss and not by their
          weights - nll is what perplexity is computed from whatever regulariser is on.
        ar, tar >= 0: AWD-LSTM's activation regularisation and temporal activation regularisation of the top layer's output (its
          --alpha and --beta; Merity, Keskar, Socher; docs/design/lm_actreg.md).  With raw (T, B, H) that output, yd its dropped
          copy (the one the head reads) and m[t,b] = (t < lengths[b]),
            loss += B (ar AR + tar TAR),  AR = sum m yd^2 / max(H #valid positions, 1),
                                          TAR = sum m[t] m[t+1] (raw[t+1] - raw[t])^2 / max(H #valid pairs, 1)
          - B times AWD-LSTM's terms, as this loss is B times the mean NLL, under both normalize settings; TAR is 0 at T == 1 or
          without a valid pair (torch's mean over no element would be NaN).  With one of them on the top layer runs without its
          own dropout and functional.activation_regularizer applies that site's dropout itself, with the factors the layer would
          have drawn - one launch forward, one backward; the head then runs as above on yd, so with the same dropout_state the nll
          part has the bits of the plain call.  A stack the library does not run with its top layer's dropout off takes the
          per-layer loop.  return_parts is then (loss, nll, smooth, z, unlikelihood, ar, tar): the two new parts are B AR and
          B TAR, detached, not multiplied by their weights, zero (and not formed) where the weight is.  With both at 0 the call
          is what it is without them, launch for launch.
        ValueError, before any device work, for eps outside [0, 1), a negative or non-finite zeta or alpha, another normalize,
        lengths that are not (B) integers, negatives of the wrong type, shape or K, and an ar or tar that is negative, not finite
        or a bool.  No value is read back from the device."""
        from .functional import check_actreg, lm_head_loss
        check_actreg(ar, tar)
        if ar > 0 or tar > 0:
            return self._regularized_loss(x, y, states, lengths, label_smoothing, z_loss, unlikelihood, negatives, normalize, return_parts,
                                          ar, tar)
        if (lengths is None and negatives is None and not return_parts and normalize == "rows"
                and label_smoothing == 0.0 and z_loss == 0.0 and unlikelihood == 0.0
                and not any(isinstance(v, bool) for v in (label_smoothing, z_loss, unlikelihood))):
            tied = self._tied_gradient(x)
            h, states = self.features(x, states) if tied is None else self._features(x, states, grad_from=tied)[:2]
            return lm_head_loss(h, self.fc.w, self.fc.b, y, grad_to=tied), states
        from .functional import check_lengths, check_objective, context_negatives, lm_head_objective_loss, objective_negatives
        check_objective(label_smoothing, z_loss, unlikelihood, normalize)
        check_lengths(lengths, x.size(1), "Model.loss")
        if unlikelihood > 0:
            negatives = objective_negatives(context_negatives(x) if negatives is None else negatives, x.numel())
        tied = self._tied_gradient(x)
        h, states = self.features(x, states) if tied is None else self._features(x, states, grad_from=tied)[:2]
        loss = lm_head_objective_loss(h, self.fc.w, self.fc.b, y, lengths=lengths, label_smoothing=label_smoothing, z_loss=z_loss,
                                      unlikelihood=unlikelihood, negatives=negatives, normalize=normalize, return_parts=return_parts,
                                      grad_to=tied)
        return loss, states

    def distill_loss(self, x, y, states, teacher, *, alpha=0.5, temperature=2.0, teacher_states=None, top=0, return_parts=False):
        """loss() with a soft-target term: this model, the student, is trained against a teacher's output distribution as well as
        against the corpus (knowledge distillation; Hinton, Vinyals, Dean) - how a low-rank Model gets close to its dense or
        wide-rank parent.  loss = scale sum_r ((1 - alpha) hard_r + alpha tau^2 KL(P_r || softmax(z_r / tau))), tau = temperature,
        hard_r what loss() charges, scaled as loss() scales (functional.lm_head_distill_loss: on a HIP device both terms and the
        gradient of their mix come from one pass over the scores, which are never handed out).  The student's features, dropout
        included, run as in loss().  The teacher is a constant; alpha == 0 is loss() and leaves a teacher tensor unread.
        teacher is
          - a (T, B, V) or (T B, V) fp32 score tensor, or a pair (top_tokens (T, B, k) int64, top_scores (T, B, k) fp32) as
            score(top=k) returns them (k <= 32; P is then softmax(top_scores / tau) on those tokens, zero elsewhere) - an offline
            teacher: returns (loss, states);
          - a module with forward(x, states) -> (scores, states) - any Model, nn.LSTM layers included: it runs on x in eval mode
            without autograd, every module's train / eval flag restored whatever is raised, from teacher_states (default:
            teacher.state_init(B)): returns (loss, states, teacher_states), the latter to hand back in with the next minibatch.
            top=k > 0 reduces the teacher to its k best tokens per position - on a HIP device through its own
            score(x, y, states=teacher_states, top=k), so no (T B, V) teacher matrix exists beyond score()'s chunk; on the CPU by
            torch.topk of its scores.
        return_parts=True: loss is the triple (loss, hard, soft), the parts detached.
        ValueError, before any device work, for alpha outside [0, 1], a temperature that is not finite and positive, top outside
        [0, 32] or given with a teacher that is not a module, and teacher tensors of the wrong shape or type.  That a row's top
        tokens are distinct and inside the vocabulary is the caller's responsibility: no value is read back from the device."""
        from .functional import check_distill, lm_head_distill_loss
        check_distill(alpha, temperature, top)
        module = isinstance(teacher, nn.Module)
        if top and not module:
            raise ValueError("vmlmf_amd: top reduces a teacher module; a teacher given as tensors is taken as it is")
        if module:
            if teacher_states is None:
                teacher_states = teacher.state_init(x.size(1))
            if top and x.is_cuda and hasattr(teacher, "score"):
                _, _, tokens, logprobs, teacher_states = teacher.score(x, y, states=teacher_states, top=top)
                teacher = (tokens, logprobs)
            else:
                flags = [(m, m.training) for m in teacher.modules()]
                try:
                    teacher.eval()
                    with torch.no_grad():
                        scores, teacher_states = teacher(x, teacher_states)
                finally:
                    for m, was in flags:
                        m.training = was
                teacher = scores
                if top:
                    values, tokens = scores.topk(top, dim=-1)
                    teacher = (tokens.reshape(*x.shape, top), values.reshape(*x.shape, top))
        else:
            from .functional import distill_teacher
            distill_teacher(teacher, x.numel(), self.vocab_size, self.fc.w.dtype)
        tied = self._tied_gradient(x)
        h, states = self.features(x, states) if tied is None else self._features(x, states, grad_from=tied)[:2]
        loss = lm_head_distill_loss(h, self.fc.w, self.fc.b, y, teacher, alpha=alpha, temperature=temperature, return_parts=return_parts,
                                    grad_to=tied)
        return (loss, states, teacher_states) if module else (loss, states)

    def _regularized_loss(self, x, y, states, lengths, label_smoothing, z_loss, unlikelihood, negatives, normalize, return_parts, ar, tar):
        """loss() with ar or tar on: the top layer's raw output, functional.activation_regularizer with that site's dropout, the head
        on the dropped copy."""
        from .functional import (activation_regularizer, activation_regularizer_stock, check_lengths, check_objective, context_negatives,
                                 lm_head_loss, lm_head_objective_loss, locked_site, objective_negatives)
        check_objective(label_smoothing, z_loss, unlikelihood, normalize)
        check_lengths(lengths, x.size(1), "Model.loss")
        if unlikelihood > 0:
            negatives = objective_negatives(context_negatives(x) if negatives is None else negatives, x.numel())
        tied = self._tied_gradient(x)
        raw, states, site = self._features(x, states, raw_top=True, grad_from=tied)
        B = x.size(1)
        if site is None or len(site) >= 4:       # no dropout at that site / the package's, inside the regulariser's launches
            p, snap, index, desc = (site or (0.0, None, 0, None))[:4]
            if site is not None and len(site) > 4:       # locked_dropout: the flag rides in the site, as in the C ABI
                index = locked_site(index)
            h, penalty, parts = activation_regularizer(raw, ar=ar, tar=tar, p=p, snap=snap, site=index, lengths=lengths, layer_desc=desc,
                                                       batch_scale=B)
        else:                                    # nn.Dropout's / LockedDropout's factors (CPU tensors, stock_dropout): the rule in stock ops
            factors = self._site_dropout(torch.ones_like(raw[:1] if self.locked_dropout else raw), site[0])
            h, penalty, parts = activation_regularizer_stock(raw, ar=ar, tar=tar, factors=factors, lengths=lengths, batch_scale=B)
        plain = (lengths is None and negatives is None and not return_parts and normalize == "rows" and label_smoothing == 0.0
                 and z_loss == 0.0 and unlikelihood == 0.0)
        if plain:
            return lm_head_loss(h, self.fc.w, self.fc.b, y, grad_to=tied) + penalty, states
        head = lm_head_objective_loss(h, self.fc.w, self.fc.b, y, lengths=lengths, label_smoothing=label_smoothing, z_loss=z_loss,
                                      unlikelihood=unlikelihood, negatives=negatives, normalize=normalize, return_parts=return_parts,
                                      grad_to=tied)
        if not return_parts:
            return head + penalty, states
        return (head[0] + penalty, *head[1:], *parts), states

    def features(self, x, states):
        """Everything of forward() in front of the vocabulary projection (vmlmf_lm.py:434-439): (T, B, H) activations, states.
        Training with p > 0 on a HIP device: the three dropouts run without mask tensors (functional.dropout_*: Philox factors
        regenerated in the backward) - the embedding's inside its gather, a VMLMF layer's inside the layer's launches; with
        self.stock_dropout = True they are nn.Dropout's launches as in the reference.  embed_dropout > 0 adds the word dropout of
        the table to the same gather (training mode only)."""
        return self._features(x, states)[:2]

    def _top_layer_desc(self, T, B):
        """The descriptor of the top layer where its own launches would apply its dropout (vmlmf_dropout_fused: the column map of
        its factors is then the kernels'), else None (identity columns)."""
        rnn = self.rnns[-1]
        if not isinstance(rnn, (MyVMLSTM, MyVMLSTMGroup)):
            return None
        import ctypes
        ur = list(rnn.u_ranks) if isinstance(rnn.u_ranks, (list, tuple)) else [rnn.u_ranks]
        desc = _lib.make_desc(rnn.variant, B, T, rnn.input_size, rnn.hidden_size, rnn.w_rank, ur, g=getattr(rnn, "g", 1), time_major=True,
                              training=True)
        return desc if _lib.lib().vmlmf_dropout_fused(ctypes.byref(desc)) == 1 else None

    def _features(self, x, states, raw_top=False, grad_from=None):
        """features(), written once.  raw_top=True (loss() under ar / tar): the top layer runs without the dropout behind it and a
        third element says what the caller applies in its place: None (eval mode, p == 0), (p, snapshot, site, layer descriptor or
        None) for functional.activation_regularizer - with a fifth element, True, under locked_dropout -, or (p,) where the
        dropouts are stock ops'.  Site i's rate is site_rates()[i]; a site whose rate is 0 is skipped."""
        rates = self.site_rates()
        locked = self.locked_dropout
        last = len(self.rnns) - 1
        word_p = self.embed_dropout if self.training else 0.0
        if (max(rates) > 0 or word_p > 0) and x.is_cuda and not getattr(self, "stock_dropout", False):
            from .functional import dropout, dropout_advance, embedding_dropout
            snap = dropout_advance(self.dropout_state())
            T, B = x.shape
            form = (True,) if locked else ()     # (three-tuples are the per-element form, as before there was another)
            x = embedding_dropout(self.embed.w, x, rates[0], snap, 0, word_p=word_p, grad_from=grad_from, locked=locked)
            top = rates[last + 1]
            site = (top, snap, last + 1, self._top_layer_desc(T, B)) + form if (raw_top and top > 0) else None
            drops = [None if (raw_top and i == last) or not rates[i + 1] > 0 else (rates[i + 1], snap, i + 1) + form
                     for i in range(len(self.rnns))]
            stacked = self._stack(x, states, drops=drops)     # (all None: a stack that needs no dropout - it still runs stacked)
            if stacked is not None:       # every layer in one launch per direction, the dropouts behind them inside it
                x, new_states = stacked
                for i, st in enumerate(new_states):
                    states[i] = st
                return x, states, site
            for i, rnn in enumerate(self.rnns):
                if isinstance(rnn, (MyVMLSTM, MyVMLSTMGroup)):
                    x, states[i] = rnn(x, states[i], drop=drops[i])
                else:
                    x, states[i] = rnn(x, states[i])
                    if drops[i] is not None:
                        x = dropout(x, rates[i + 1], snap, i + 1, locked=locked)
            return x, states, site
        site = (rates[last + 1],) if (raw_top and rates[last + 1] > 0) else None
        if word_p > 0:                           # CPU tensors, stock_dropout: AWD-LSTM's embedded_dropout in stock ops
            from .functional import embedding_dropout_stock
            x = self._site_dropout(embedding_dropout_stock(self.embed.w, x, 0.0, word_p), rates[0]) if locked else \
                embedding_dropout_stock(self.embed.w, x, rates[0], word_p)
        elif grad_from is not None:
            from .functional import embedding
            x = self._site_dropout(embedding(self.embed.w, x, grad_from=grad_from), rates[0])
        else:
            x = self.embed(x)
            x = self._site_dropout(x, rates[0])
        stacked = self._stack(x, states)
        if stacked is not None:
            x, new_states = stacked
            for i, st in enumerate(new_states):
                states[i] = st
            if not raw_top:
                x = self._site_dropout(x, rates[last + 1])
        else:
            for i, rnn in enumerate(self.rnns):
                x, states[i] = rnn(x, states[i])
                if not (raw_top and i == last):
                    x = self._site_dropout(x, rates[i + 1])
        return x, states, site

    def dropout_state(self, seed=None):
        """{seed, offset} of this model's dropout generator on its device (created on first use; seed=None draws it from torch's CPU
        generator).  Create it BEFORE capturing a training step into a hipGraph (any eager warm-up step does)."""
        dev = self.embed.w.device
        st = getattr(self, "_drop_state", None)
        if st is None or st.device != dev or seed is not None:
            from .functional import dropout_state
            st = self._drop_state = dropout_state(dev, seed)
        return st

    def sampler_state(self, seed=None):
        """{seed, offset} of the generator generate() samples from - its own, apart from the dropout generator, so sampling leaves
        training's masks where they were (created on first use; seed=None draws it from torch's CPU generator; a seed re-seeds)."""
        dev = self.embed.w.device
        st = getattr(self, "_sample_state", None)
        if st is None or st.device != dev or seed is not None:
            from .functional import dropout_state
            st = self._sample_state = dropout_state(dev, seed)
        return st

    def generate(self, prompt, steps, states=None, temperature=1.0, seed=None, chunk=None, layer_path="layers", top_k=None, top_p=None,
                 eos=None, min_length=0, repetition_penalty=1.0, logit_bias=None, banned_tokens=None, return_lengths=False,
                 no_repeat_ngram_size=0, banned_sequences=None, frequency_penalty=0.0, presence_penalty=0.0, *, min_p=None, typical_p=None,
                 epsilon_cutoff=None, eta_cutoff=None, automaton=None, automaton_state=None):
        """Continue `prompt` (T0, B) int64 - time-major as lm_test.minibatch - by `steps` tokens per row.  Returns (tokens (steps, B)
        int64, logprobs (steps, B), states); logprobs are the untempered log-softmax of the chosen tokens (what nll_loss charges), states
        have taken in the prompt and every generated token (Model.forward over torch.cat([prompt, tokens]) ends in the same states).
        The prompt runs once through features() without dropout; each further token is one vmlmf_lm_sample launch (decoding.lm_sample)
        and the layers at T = 1.  temperature 0: greedy; tau > 0: softmax(scores / tau) draws from sampler_state() (seed: re-seed it
        first), snapshotted and advanced once per call - the same seed gives the same tokens, the next call fresh ones.
        chunk=K (steps % K == 0): the decode steps run as a captured hipGraph of K steps (DecodeGraph), replayed steps / K times, the
        generator snapshotted and advanced once per REPLAY (the eager form: once per call) - so with one seed the chunked and the eager
        form draw the same first K tokens and different ones after them; greedy decoding is the same either way.  layer_path: "layers"
        (one call per layer on kept parameter images; the default) or "stack" (stack_layers' one launch where it covers the layers;
        measured at the PTB size: docs/design/lm_sampling.md).  Every module's train / eval flag is as the caller left it afterwards.
        top_k / top_p cut the tail of the tempered distribution before the draw: temperature first, then the top_k tokens with the
        largest scores (equal scores: the lower index first), then of those the shortest prefix whose renormalised mass reaches top_p
        (decoding.lm_sample; None, top_k = 0 and top_p = 1.0: off; ValueError for top_k < 0 and top_p outside (0, 1]).  The generator
        is snapshotted and advanced exactly as without them, so a filtered and an unfiltered call from one seed see the same noise;
        logprobs stay those of the unfiltered distribution; greedy decoding is unchanged.
        Stopping and token controls (all off by default; with any of eos, repetition_penalty != 1, logit_bias, banned_tokens given the
        choice of every step is ONE launch of a library of its own behind the head's GEMM - vmlmf_decode_choose, include/vmlmf_decode.h -
        and without them this is the call above, launch for launch).  Per step and row, on the fp32 scores x, in this order:
        repetition_penalty = theta > 0 turns the score of a token the row has held - prompt included - into x / theta (x > 0) or x theta
        (Keskar et al., CTRL); logit_bias (V) fp32, entries finite or -inf, is added (banned_tokens: indices, shorthand for -inf); while a
        row has emitted fewer than min_length tokens eos is held at -inf; then temperature, top_k, top_p and the draw as above, on the
        same noise - a token at -inf is never chosen.  A row that has emitted eos is finished: its later tokens are eos with
        log-probability 0, which the layers keep taking in (the states cover the padding, as beam_search's).  logprobs stay the
        unprocessed log-softmax.  Decoding always runs the full `steps`: the step loop has no host synchronisation.
        return_lengths=True: (tokens, logprobs, lengths (B) int32 - tokens up to and including eos -, states).  ValueError, before any
        device work, for repetition_penalty <= 0 or not finite, min_length < 0 or without eos, eos or a banned index outside the
        vocabulary, a logit_bias that is not (V) fp32, holds NaN or +inf (its values are read back once), or leaves nothing to choose.
        History controls (all off by default; with any of no_repeat_ngram_size, banned_sequences, frequency_penalty, presence_penalty
        given the choice of every step is ONE launch of a fourth library behind the head's GEMM - vmlmf_history_choose,
        include/vmlmf_history.h -, which applies the controls above too; without them this is the call above, launch for launch, and
        that library is never opened).  Beside a row's set of tokens the launch keeps its sequence - prompt included - and how often it
        has GENERATED each token (the prompt is not counted; the count saturates at 65535).  Per step and row, in this order:
        repetition_penalty as above, r; then q = (r - frequency_penalty * count) - (presence_penalty if count > 0 else 0), in fp32,
        each operation rounded, both penalties finite and >= 0; then logit_bias and min_length as above; then the history bans, to
        -inf: no_repeat_ngram_size = n >= 1 closes every token that would complete an n-gram the row already holds (the tokens that
        followed an earlier occurrence of its last n - 1 tokens; n = 1: every token of the history; overlapping occurrences count -
        the rule of Hugging Face's NoRepeatNGramLogitsProcessor); banned_sequences, a list of lists of tokens, closes a sequence's
        last token while the row ends in the tokens before it (a sequence of one token is always closed).  Then temperature, top_k,
        top_p and the draw as above on the same noise; logprobs stay the unprocessed log-softmax.  Bans need a vocabulary of at most
        65536 tokens (a row's ban set is a bitmap in the workgroup's LDS); the penalties do not.  ValueError, before any device work,
        for a negative n, a negative or non-finite penalty, an empty sequence or one with a token outside the vocabulary, more than
        4096 sequence tokens in all, and - with a ban on - for a vocabulary that might run out of open tokens: V must exceed the tokens
        the other controls close + the prompt's length + steps + the number of sequences + 1.
        Truncation samplers - min_p, typical_p, epsilon_cutoff, eta_cutoff, keyword-only - (all off by default: None, and min_p = 0, typical_p = 1.0, a cutoff of 0; with any of them on the choice
        of every step is ONE launch of a library of its own behind the head's GEMM - vmlmf_truncate_choose,
        include/vmlmf_truncate.h - which runs top_k and top_p too; without them this is the call above, launch for launch, and that
        library is never opened).  They act on the tempered score z = c / tau - c the raw score, or the controlled score when eos,
        repetition_penalty, logit_bias or banned_tokens are on -, in Hugging Face's order behind temperature, top_k and top_p, each on
        the distribution renormalised over the survivors of the stages before it, each keeping at least its own first token, a token
        at -inf never kept: min_p = a in (0, 1] keeps the tokens with p >= a p_max (every tie in); typical_p = m in (0, 1) orders
        the survivors by |-log p - entropy|, smaller first, equal ones to the lower index, and keeps the shortest prefix whose mass
        reaches m (locally typical sampling, Meister et al.; the band need not hold the most probable token); epsilon_cutoff keeps
        the tokens with p >= epsilon, eta_cutoff those with p >= min(eta, sqrt(eta) exp(-entropy)) (Hewitt et al.), both always the
        most probable survivor.  The draw is the argmax over the kept set on the noise of the untruncated call; logprobs stay the
        unprocessed log-softmax; greedy decoding accepts them and is unchanged.  The choice is exact and repeats bit for bit.
        ValueError, before any device work, for a value outside those ranges and for any of them together with the history controls
        (no_repeat_ngram_size, banned_sequences, frequency_penalty, presence_penalty): that composition is out of scope.
        Token automaton - automaton, automaton_state, keyword-only - (off by default: None; with automaton= the choice of every step is ONE launch of a library of its own behind the head's GEMM -
        vmlmf_automaton_choose, include/vmlmf_automaton.h -; without it this is the call above, launch for launch, and that library is
        never opened).  automaton: a vmlmf_amd.TokenAutomaton over the vocabulary - a dense table next (S, V) on the device, next[s][v]
        >= 0: in state s token v is open and leads to that state; forced, one_of, template and avoiding build the usual ones.  Every row
        carries one state; per step, behind logit_bias and min_length, the tokens the row's state does not offer go to -inf, and the
        state moves on with the chosen token.  automaton_state: (B) int32 start states, default automaton.start for every row - the
        prompt is NOT consumed: pass automaton.advance(prompt) where it should be.  It composes with temperature, top_k, top_p, eos,
        min_length, repetition_penalty, logit_bias, banned_tokens, return_lengths and chunk; the noise is the plain call's and logprobs
        stay the unprocessed log-softmax.  ValueError, before any device work, for an automaton over another vocabulary, an
        automaton_state of another shape or dtype or with a state outside [0, S), a state that can be reached from the start states (not
        through eos, when eos is given) and has no token left that banned_tokens and -inf biases leave open - with min_length > 0: none
        besides eos -, and for the automaton together with a history control or a truncation sampler: those compositions are out of
        scope."""
        from . import decoding
        return decoding.generate(self, prompt, steps, states, temperature, seed, chunk, layer_path, top_k, top_p, eos, min_length,
                                 repetition_penalty, logit_bias, banned_tokens, return_lengths, no_repeat_ngram_size, banned_sequences,
                                 frequency_penalty, presence_penalty, min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff,
                                 eta_cutoff=eta_cutoff, automaton=automaton, automaton_state=automaton_state)

    def beam_search(self, prompt, steps, beams=4, states=None, eos=None, length_penalty=0.0, chunk=None, min_length=0, banned_tokens=None,
                    no_repeat_ngram_size=0, banned_sequences=None, *, automaton=None, automaton_state=None):
        """Continue `prompt` (T0, B) int64 by `steps` tokens along the `beams` (W) most probable hypotheses per row.  Returns (tokens
        (steps, B, W) int64, scores (B, W) fp32, lengths (B, W) int32, states): tokens[:, b, w] is hypothesis w of row b, best first;
        its score is the fp32 sum of the untempered log-softmax (bias included) of its tokens - what nll_loss charges -; states are per
        layer (h, c) of (B W, H), row b W + w, after every returned token of the hypothesis (Model.forward over
        torch.cat([prompt, tokens[:, b, w]]) ends in them).
        The prompt runs once through features() without dropout.  Beam 0 of each row then starts at score 0, beams 1 .. W - 1 at -inf,
        all on the prompt's state.  A step keeps the W best of a row's candidates under one total order - larger total first, equal
        totals to the lower flat index w V + v - and leaves them in that order (decoding.lm_beam_step: one launch behind the head's
        GEMM; a second launch reorders the layers' states, then the layers run at T = 1 on kept parameter images).
        eos: a beam that has emitted it is finished - it offers (w, eos) alone at its score so far, its length stops growing and its
        later tokens are eos (which the layers keep taking in: the states cover the padding).  None: no beam ever finishes.
        length_penalty = a > 0: the W hypotheses of a row are finally re-sorted by score / length ** a, stably, best first; scores stay the
        raw sums.  Decoding always runs the full `steps`: an early exit would need a host synchronisation, and the step loop has none.
        chunk=K (steps % K == 0): K steps are captured into a linear hipGraph on one stream and replayed steps / K times (BeamGraph):
        the eager call's bits.  ValueError for beams < 1, beams > 32 and beams > V; no random generator is touched; every module's
        train / eval flag is as the caller left it afterwards.
        min_length, banned_tokens, no_repeat_ngram_size, banned_sequences: generate()'s controls of the same names, per HYPOTHESIS - a
        live beam does not offer eos before it has emitted min_length tokens (needs eos), never a banned token, never a token that
        would repeat an n-gram of its prompt and tokens so far, never the last token of a banned sequence whose other tokens it ends
        in.  They only close candidates: a closed candidate is not offered at all, every offered one keeps its total, so scores stay
        the sums of plain log-probabilities; a finished beam keeps offering eos.  With any of them on the selection is the controlled
        launch (decoding.BeamControls, vmlmf_beamctl_step) and, for the last two, one small launch in front of it that forms every
        beam's ban set from its history (vmlmf_history_bans on B W rows); without them the call is launch for launch what it was.
        ValueError for what generate() refuses for the same arguments, for eos among banned_tokens, and for a vocabulary in which a
        beam might run short of candidates: V < closed + T0 + steps + len(banned_sequences) + beams.
        automaton, automaton_state (keyword-only): generate()'s of the same names, per HYPOTHESIS: every beam
        carries a state of the vmlmf_amd.TokenAutomaton, a live beam offers only what its state's table row opens, a survivor's state is
        its parent's moved on by its token (a finished parent's: unchanged).  The selection is then ONE launch of
        vmlmf_automaton_beam_step (include/vmlmf_automaton.h: the same kernel under a third offer policy); the beams' states travel with
        cum, finished and length, through chunk= too.  It composes with eos, min_length, banned_tokens, length_penalty and chunk;
        ValueError together with no_repeat_ngram_size or banned_sequences, and for what generate() refuses of the automaton.  A
        constraint that admits fewer than `beams` sequences leaves the surplus hypotheses at score -inf: they repeat admitted ones,
        continued from the beams that start at -inf.  Without automaton= the call is launch for launch what it was."""
        from . import decoding
        return decoding.beam_search(self, prompt, steps, beams, states, eos, length_penalty, chunk, min_length, banned_tokens,
                                    no_repeat_ngram_size, banned_sequences, automaton=automaton, automaton_state=automaton_state)

    def group_beam_search(self, prompt, steps, beams=4, *, groups=2, diversity_penalty=0.5, states=None, eos=None, length_penalty=0.0,
                          chunk=None):
        """Diverse beam search (Vijayakumar et al., "Diverse Beam Search"): beam_search() whose `beams` (W) hypotheses per row are kept
        in `groups` (G, dividing W) groups of Wg = W / G that never exchange beams, each group steered away from the tokens the groups
        before it chose in the same step.  Everything behind `beams` is keyword-only.  Returns beam_search()'s (tokens (steps, B, W)
        int64, scores (B, W) fp32, lengths (B, W) int32, states), group-major: group g owns slots g Wg .. g Wg + Wg - 1, the best
        hypothesis of each group first; scores are fp32 sums of plain log-probabilities, as beam_search()'s.
        Start: slot g Wg of every group at score 0, the other slots at -inf, all on the prompt's state.
        Step: the groups are processed in order g = 0 .. G - 1.  The beams of group g offer what they offer in beam_search() - a live
        beam w every token v at total = score[w] + log_softmax[v], a finished beam (w, eos) alone at its score so far.  A live beam's
        candidate is ranked by aug = total - diversity_penalty n, where n counts the survivors that groups 0 .. g - 1 of this row chose
        in this step with token v and a live parent (a finished beam's padding eos is not a choice and does not count); aug is formed
        in fp32 as two separately rounded operations (no fused multiply-add; for n = 0 it is the total).  A finished beam's candidate is
        not penalised.  Larger aug first, equal aug to the lower flat index w V + v (w the beam's index in the whole row); the first
        Wg candidates go to the group's slots in that order, each at its RAW total.  The penalty steers the step's choice and is never
        accumulated: this is the paper's objective.  (Hugging Face's num_beam_groups / diversity_penalty adds the penalty into the
        beam scores it carries; its scores are therefore not sums of log-probabilities, and its later steps differ.)
        One launch per step behind the head's GEMM (decoding.GroupBeams, vmlmf_beamgroup_step - beam_search()'s kernel whose merge runs
        group by group; a library of its own, opened by the first call), exact and bit-identical from run to run; the state reorder
        and the layers are beam_search()'s.  With length_penalty = a > 0 the stable re-sort by score / length ** a happens within each
        group.  chunk=K captures K steps into a hipGraph (BeamGraph): the eager call's bits.  groups=1 is beam_search() to the bit;
        diversity_penalty=0 with G > 1 gives G identical groups.
        ValueError, before any device work, for groups < 1, beams % groups != 0, a diversity_penalty that is negative or not finite,
        and for what beam_search() refuses of beams, eos, length_penalty, steps and chunk.  There are no token controls and no
        automaton here."""
        from . import decoding
        return decoding.group_beam_search(self, prompt, steps, beams, groups=groups, diversity_penalty=diversity_penalty, states=states,
                                          eos=eos, length_penalty=length_penalty, chunk=chunk)

    def contrastive_search(self, prompt, steps, top_k=4, penalty_alpha=0.6, *, states=None, eos=None, chunk=None, return_penalties=False):
        """Contrastive search (Su et al., "A Contrastive Framework for Neural Text Generation"; Hugging Face's penalty_alpha / top_k):
        the deterministic decoder that weighs a candidate's probability against its similarity with what the row has already said, and
        so does not fall into the repetition loops of greedy and beam decoding.  Continue `prompt` (T0, B) int64, T0 >= 1, by `steps`
        tokens per row; everything behind penalty_alpha is keyword-only.  Returns (tokens (steps, B) int64, logprobs (steps, B),
        lengths (B) int32, states) - with return_penalties=True (tokens, logprobs, lengths, penalties (steps, B), states).
        Per step and row b: (1) the candidates are the k = top_k most probable tokens in the project's one total order (larger score
        first, equal scores to the lower index; Model.score's selection, vmlmf_score_rows), p_j = exp(logprob_j) under the WHOLE
        distribution; (2) every candidate is embedded and taken through the layers at T = 1 from the row's states (B k rows), h_j the
        top layer's output; (3) s_j = the largest cosine of h_j with the row's history - the top layer's outputs behind every prompt
        token, the last included, and behind every token chosen so far; a zero vector has cosine 0 with everything; (4) j* = argmax_j
        (1 - penalty_alpha) p_j - penalty_alpha s_j in fp32, equal values to the lower j, a NaN value loses to every number; (5) the
        token is candidate j*'s, its logprob the plain log-softmax (what score() and generate() report for it), penalties hold s_j*;
        h_j* goes behind the history and to the next head GEMM, the states follow candidate j*.  Steps (3) to (5) are ONE launch
        (decoding.lm_contrast_step: vmlmf_contrast_choose, include/vmlmf_contrast.h; a library of its own, opened by the first call)
        that reads the row's history once; its results are the same bits from run to run.  penalty_alpha = 0 and top_k = 1 are greedy
        decoding.
        eos: a row that emits it is finished - it is padded with eos at log-probability 0, its history stops growing; lengths count
        the tokens up to and including eos (`steps` where none came).  Decoding always runs the full `steps`.
        states (default: state_init) are taken in front of the prompt; the returned states have taken in the prompt and tokens[:-1] -
        everything but the last token, so a further call continues from them with tokens[-1:] as its prompt (Model.forward over
        torch.cat([prompt, tokens[:-1]]) ends in them; with steps = 0 they are the prompt's).  A finished row's states are not
        meaningful.  chunk=K (steps % K == 0): K steps are captured into a hipGraph (decoding.ContrastGraph) and replayed steps / K
        times, the history's length living on the device: the eager call's bits.  No random generator is touched; every module's
        train / eval flag is as the caller left it afterwards.
        ValueError, before any device work, for top_k outside [1, min(16, V)], a penalty_alpha outside [0, 1] or not finite, a hidden
        size whose top_k candidates exceed the kernel's LDS budget (top_k * 4 * ceil(H / 4) > 14336), T0 < 1, eos outside [0, V), steps
        < 0 and a chunk that does not divide steps; RuntimeError for CPU tensors.  There are no token controls, filters or automata
        here: that composition is out of scope."""
        from . import decoding
        return decoding.contrastive_search(self, prompt, steps, top_k, penalty_alpha, states=states, eos=eos, chunk=chunk,
                                           return_penalties=return_penalties)

    def stochastic_beam_search(self, prompt, steps, beams=4, *, seed=None, states=None, eos=None, chunk=None):
        """Stochastic beam search (Kool, van Hoof and Welling, "Stochastic Beams and Where to Find Them", ICML 2019): `beams` (W)
        DIFFERENT continuations of each row of `prompt` (T0, B) int64, drawn as an exact sample without replacement from the model's
        distribution over sequences of `steps` tokens - what repeating generate() cannot give (it repeats itself) and beam_search()
        is not (it is no sample).  Everything behind `beams` is keyword-only.  Returns (tokens (steps, B, W) int64, scores (B, W)
        fp32, perturbed (B, W) fp32, lengths (B, W) int32, states), the hypotheses of a row in order of `perturbed`, largest first:
        scores are fp32 sums of plain log-probabilities, as beam_search()'s; the first k hypotheses of a row are a sample without
        replacement of size k, in the order of the draw; with beams = k + 1 the last `perturbed` is the threshold kappa of the paper's
        estimators (a hypothesis s of the first k has inclusion probability q = 1 - exp(-exp(score_s - kappa))).
        Start: beam 0 of every row at score 0 and perturbed value 0, the other beams at -inf, all on the prompt's state.
        Step (one launch behind the head's GEMM: decoding.lm_sbeam_step, vmlmf_sbeam_step; include/vmlmf_sbeam.h has the contract; a
        library of its own, opened by the first call).  A live beam w of row b with score cum and perturbed value T offers every
        token v at phi = cum + log_softmax[v] - beam_search()'s fp32 total, to the bit - perturbed to gt = phi + Gumbel noise, the
        sampler's counter-based noise (Philox4x32-10 under a snapshot of sampler_state()) at position draw B W + b W + w, draw the
        number of steps taken, counted on the device.  With Z = max_v gt the candidate's perturbed value is G = T where gt == Z and
        otherwise G = T - max(u, 0) - log1p(exp(-|u|)), u = T - gt + log1p(-exp(gt - Z)): the noise drawn top-down, so the largest
        child inherits its parent's value and no child exceeds it.  A finished beam offers (w, eos) alone at its score and value.
        The W candidates of a row with the largest G survive, equal G to the lower flat index w V + v, in that order; the state
        reorder and the layers are beam_search()'s.  With beams = 1 the tokens are generate(temperature=1.0)'s for the same seed
        wherever fp32 rounding does not decide (the noise is the same; generate adds it to the raw score, this to the
        log-probability).
        seed follows generate(): it re-seeds sampler_state(), which is snapshotted and advanced ONCE per call - the same seed gives
        the same sample, the next call a fresh one.  chunk=K (steps % K == 0) captures K steps into a hipGraph
        (decoding.BeamGraph under a StochasticBeams) and replays it steps / K times; the snapshot is the call's and the step count lives on the
        device, so it gives the eager call's bits (unlike generate(chunk=K), which snapshots per replay).  The results are the same
        bits from run to run.  eos: a hypothesis that emits it is finished - padded with eos, its score and perturbed value frozen;
        lengths count the tokens up to and including eos.  Decoding always runs the full `steps`.  states (default: state_init) are
        taken in front of the prompt; the returned states are the hypotheses', rows b W + w.  Every module's train / eval flag is as
        the caller left it afterwards.
        ValueError, before any device work, for beams outside [1, min(32, V)], eos outside [0, V), steps < 0 and a chunk that does
        not divide steps; RuntimeError for CPU tensors.  There is no temperature, no token control and no automaton here: that
        composition is out of scope."""
        from . import decoding
        return decoding.stochastic_beam_search(self, prompt, steps, beams, seed=seed, states=states, eos=eos, chunk=chunk)

    def score(self, tokens, targets=None, states=None, lengths=None, top=0, chunk_rows=2048):
        """How probable a given text is, token by token.  targets=None: `tokens` is (T + 1, B) int64, time-major; the inputs are
        tokens[:-1] and the targets tokens[1:].  Otherwise tokens and targets are both (T, B) int64, as lm_test.minibatch hands them
        out.  Returns (logprobs (T, B) fp32, ranks (T, B) int32, states): logprobs[t, b] is the untempered log-softmax (bias included)
        of targets[t, b] behind inputs[:t + 1, b] - what nll_loss charges for it, and what generate and beam_search report for the
        tokens they choose -; ranks[t, b] is the number of tokens ahead of the target in the project's one total order (larger score
        first, equal scores to the lower index): 0 where greedy decoding would have chosen it.  states (default: state_init) are those
        of Model.forward over the inputs.
        top in [1, min(32, V)]: returns (logprobs, ranks, top_tokens (T, B, top) int64, top_logprobs (T, B, top), states) - the first
        `top` tokens of that order at every position, in order, and their log-probabilities.
        lengths (B) integer: positions t >= lengths[b] have no target, as has every position whose target is negative: logprob 0.0
        exactly, rank -1 (their top outputs are those of any position), so logprobs.sum(0) is a padded row's total.  lengths on the
        device keep the call free of host synchronisation (capturable); lengths on the CPU cost one blocking host-to-device copy.
        The inputs run once through features() in eval mode, without autograd and on kept parameter images, whatever mode the model is
        in; then per chunk of at most chunk_rows of the T B positions the head's GEMM and ONE launch of a library of its own
        (scoring.lm_score: vmlmf_score_rows, include/vmlmf_score.h), so no more than chunk_rows x V scores exist at a time.  Every
        module's train / eval flag and pack cache are as the caller left them afterwards, whatever is raised; no random generator is
        touched.  ValueError, before any device work, for top outside [0, min(32, V)], chunk_rows < 1, tokens that are not 2-D int64,
        targets of another shape or type, fewer than one position, and lengths that are not (B) integers; RuntimeError for CPU
        tensors.  An input token outside the vocabulary and a target >= V are the caller's errors: the call never
        reads a value back from the device, so it does not to look for them (such a target's position gives NaN and -1)."""
        from . import scoring
        return scoring.score(self, tokens, targets, states, lengths, top, chunk_rows)

    def cache_score(self, tokens, targets=None, *, theta=0.3, lam=0.1, window=500, cache=None, states=None, return_parts=False,
                    chunk_rows=2048):
        """score() under a continuous cache (Grave, Joulin and Usunier, "Improving Neural Language Models with a Continuous Cache"):
        the model's distribution mixed with one over the tokens that followed the last `window` positions, each weighted by how
        close the top layer's output behind it is to the current one - what lowers an LSTM language model's perplexity on a text
        that repeats its words, without retraining.  tokens / targets are score()'s: targets=None takes (T + 1, B) int64 tokens,
        time-major, else both are (T, B); everything behind targets is keyword-only.  Returns (logprobs (T, B) fp32, states, cache) -
        with return_parts=True (logprobs, vocab_logprobs, cache_logprobs, states, cache).
        Per row a cache holds pairs (k_j, w_j): k_j the top layer's output behind a token, w_j the token that came next.  For a
        position with output q, target y, vocabulary log-probability lv (score()'s logprobs, unchanged: scoring.lm_score) and the
        band of the last m = min(window, pairs so far) pairs strictly before it:
            s_j  = theta * dot(q, k_j)
            lc   = log(sum_{j: w_j == y} exp(s_j - M)) - log(sum_j exp(s_j - M)),  M = max_j s_j        -inf where no w_j == y
            logp = logaddexp(log1p(-lam) + lv, log(lam) + lc)
        m == 0 (an empty cache) and lam == 0 give lv's bits; no match in the band gives log1p(-lam) + lv; a band whose every token
        is y gives lc == 0.0 exactly.  The position's own pair (q, y) enters the cache after it has been scored.
        cache (default: an empty NeuralCache(B, H, device, window)) is moved on in place and returned with the states: both feed the
        next call, which is how a corpus is walked in chunks (lm_test.py's perplexity: 35 positions at a time); the chunking changes
        the results in rounding only.  A given cache must be one of this B, H and window.
        The inputs run once through features() in eval mode, without autograd and on kept parameter images; then score()'s head and,
        for the whole call, ONE launch of a library of its own (scoring.lm_cache_score: vmlmf_ncache_score, include/vmlmf_ncache.h;
        opened by the first call) behind one copy of the carried keys and the call's outputs into a (B, n + T, H) buffer.  Its
        results are the same bits from run to run.  Every module's train / eval flag is as the caller left it afterwards; no random
        generator is touched; no value is read back from the device.
        ValueError, before any device work, for a window < 1, a theta that is not finite, a lam outside [0, 1), a hidden size above
        2048, chunk_rows < 1, tokens that are not 2-D int64, targets of another shape or type, fewer than one position and a cache
        of another B, H or window; RuntimeError for CPU tensors.  A target outside [0, V) is the caller's error, as in score()."""
        from . import scoring
        return scoring.cache_score(self, tokens, targets, theta=theta, lam=lam, window=window, cache=cache, states=states,
                                   return_parts=return_parts, chunk_rows=chunk_rows)
