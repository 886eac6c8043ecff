"""vmlmf_amd: the VMLMF compressed-LSTM forward/backward hot path as hand-written HIP kernels for
MI355X (gfx950), behind the reference's own nn.Module API.

    from vmlmf_amd import MyVMLMFCell, MyVMLMFCellg2, MyLSTM, Net      # HAR   (models/vmlmf*.py)
    from vmlmf_amd import MyVMLSTM, MyVMLSTMGroup, Model               # LM    (models/vmlmf_lm.py)
    from vmlmf_amd import nll_loss                                     #       (train_test/lm_test.py)
"""
from .cells import MyVMLMFCell, MyVMLMFCellg2, MyVMLMFgCellg2, MyLSTMCell, MyLSTM, Net, TIME_STEPS, RECURRENT_MAX, RECURRENT_MIN
from .lm import MyVMLSTM, MyVMLSTMGroup, Embed, Linear, LSTM, Model
from .functional import (vmlmf_sequence, vmlmf_stack, head_linear, cross_entropy, CrossEntropyLoss, nll_loss, linear_nll, lm_head_loss, lm_head_distill_loss, lm_head_objective_loss, context_negatives, embedding, unit_gradient,
                         set_compute_dtype, cache_packed_parameters, dropout, dropout_state, dropout_advance, embedding_dropout,
                         embedding_dropout_stock, word_dropout_factors, TiedGradient, tied_gradient,
                         activation_regularizer, activation_regularizer_stock)
from .decoding import DecodeGraph, BeamGraph, DecodeControls, HistoryControls, BeamControls, Truncation, TokenAutomaton, AutomatonControls, AutomatonBeamControls, GroupBeams, ContrastControls, ContrastGraph, lm_contrast_step, StochasticBeams, StochasticBeamGraph, lm_sbeam_step, lm_sample, lm_beam_step, beam_gather, beam_backtrack
from .scoring import lm_score, NeuralCache, lm_cache_score
from . import optim
from .dyneval import DynamicEval, dyneval_step, dyneval_accumulate, dyneval_step_stock, dyneval_accumulate_stock
from .graphed import GraphedTrainStep

__all__ = ["GraphedTrainStep", "vmlmf_stack", "optim", "DynamicEval", "dyneval_step", "dyneval_accumulate", "dyneval_step_stock", "dyneval_accumulate_stock", "head_linear", "cross_entropy", "CrossEntropyLoss", "MyVMLMFCell", "MyVMLMFCellg2", "MyVMLMFgCellg2", "MyLSTMCell", "MyLSTM", "Net", "MyVMLSTM", "MyVMLSTMGroup",
           "Embed", "Linear", "LSTM", "Model", "DecodeGraph", "BeamGraph", "lm_beam_step", "beam_gather", "beam_backtrack", "nll_loss", "linear_nll", "lm_head_loss", "lm_head_distill_loss", "lm_head_objective_loss", "context_negatives", "embedding", "unit_gradient", "vmlmf_sequence", "dropout", "dropout_state", "dropout_advance", "lm_sample",
           "embedding_dropout", "embedding_dropout_stock", "word_dropout_factors", "TiedGradient", "tied_gradient", "activation_regularizer", "activation_regularizer_stock", "DecodeControls", "HistoryControls", "BeamControls", "lm_score", "Truncation", "TokenAutomaton", "AutomatonControls",
           "AutomatonBeamControls", "GroupBeams", "ContrastControls", "ContrastGraph", "lm_contrast_step", "StochasticBeams", "StochasticBeamGraph",
           "lm_sbeam_step", "NeuralCache", "lm_cache_score"]
