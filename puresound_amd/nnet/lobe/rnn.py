"""Recurrent lobes (mirror of puresound/nnet/lobe/rnn.py:9-55): SingleRNN holds an nn.LSTM (or nn.GRU / nn.RNN) and its projection under
the reference's keys (`rnn.*`, `proj.*`).  The dual-path blocks of DPCRN / DPARN drive its LSTM through _plans.lstm_path
with their own strided walks; as a layer of its own (the speaker net of tse_skim_v1_causal, egs/tse/model.py:487-495)
it runs one sequence per utterance over the frame axis: input projection GEMM, recurrence, output projection GEMM, on the
kernels _plans.lstm_route(standalone=True) names."""
import torch
import torch.nn as nn

from ... import hip
from ...ops import op_module, same_shape
from .._plans import GemmPlanCache, linear_plan, lstm_gates, lstm_plan, lstm_recurrence, lstm_route, packed, rnn_plan


@op_module("single_rnn_fwd", same_shape)
class SingleRNN(GemmPlanCache, nn.Module):
    def __init__(self, rnn_type: str, input_size: int, hidden_size: int, bidirectional: bool = False,
                 dropout: float = 0.0):
        super().__init__()
        rnn_type = rnn_type.upper()
        assert rnn_type in ["RNN", "LSTM", "GRU"], f"Only support 'RNN', 'LSTM' and 'GRU', current type: {rnn_type}"
        self.rnn_type = rnn_type
        self.input_size = input_size
        self.hidden_size = hidden_size
        self.num_direction = int(bidirectional) + 1
        self.rnn = getattr(nn, rnn_type)(input_size, hidden_size, 1, batch_first=True, bidirectional=bidirectional)
        self.drop = nn.Dropout(p=dropout)
        self.proj = nn.Linear(hidden_size * self.num_direction, input_size)

    def _build(self, device):
        if self.training and self.drop.p > 0:
            raise RuntimeError("SingleRNN: dropout is active; the HIP path is inference only -- call .eval()")
        if self.rnn_type != "LSTM":   # GRU / RNN: the plain kernel (ps_rnn_f32): no recipe builds them
            return dict(rnn=rnn_plan(self.rnn, device), proj=linear_plan(self.proj, device))
        return dict(rnn=lstm_plan(self.rnn, device, self.gemm_precision), proj=linear_plan(self.proj, device))

    def forward_padded(self, x: torch.Tensor, t: int, t_rows=None) -> torch.Tensor:
        """padded [N, C, ldt] -> [N, C, ldt]: proj(LSTM(x)) over the t frames of each utterance (lobe/rnn.py:37-55).
        t_rows (int32 [N] on the device; a ragged batch, LSTM only): utterance n holds t_rows[n] frames and anything behind
        them, which is never read as data: the recurrence is hip.lstm_rows, whose backward pass starts at the row's own last
        frame, and row n's first t_rows[n] frames are the utterance's own (behind them: the projection's bias)."""
        p = self._plan_get(x.device, self._build)
        rnn, proj = p["rnn"], p["proj"]
        n, _, ldt = x.shape
        if t_rows is not None and self.rnn_type != "LSTM":
            raise NotImplementedError("SingleRNN: a per-row frame limit for the LSTM only")
        if self.rnn_type != "LSTM":
            gx, _ = hip.conv1x1(x, t, rnn["wih"], rnn["rows"], None, rnn["bias"],
                                out=torch.empty(n, rnn["rows"], ldt, dtype=torch.float32, device=x.device))
            hseq = hip.rnn(gx, rnn["whh_t"], rnn["kind"], rnn["H"], rnn["D"], 1, ldt, t, 1, rnn["bhn"])
            y, _ = hip.conv1x1(hseq, t, proj["wt"], proj["M"], None, proj["bias"],
                               out=torch.empty(n, proj["M"], ldt, dtype=torch.float32, device=x.device))
            return y
        # one sequence per utterance: q = 1, the steps walk the frame axis (the bidirectional 192-unit LSTM over the enrolment
        # of tse_skim_v1: 4000 dependent steps); _plans.lstm_route(standalone=True) says which kernels run
        route = lstm_route(rnn, n, ldt, t, (1, ldt, t, 1), standalone=True)
        gx = lstm_gates(x, t, rnn, route)
        hseq, _ = lstm_recurrence(gx, x, t, rnn, route.kernel, (1, ldt, t, 1), steps_rows=t_rows)
        y = torch.empty(n, proj["M"], ldt, dtype=torch.float32, device=x.device)
        if route.layout == "fmajor":   # the fp16x2 arithmetic all the way: h is an LSTM output, |h| < 1 is its range
            wf, we = packed(proj, "f16x2", hip.pack_wt_f16x2, proj["w_rows"])
            hip.conv1x1_f16x2(hseq, t, wf, we, proj["M"], None, proj["bias"], x_bound=1.0, out=y)
        else:
            hip.conv1x1(hseq, t, proj["wt"], proj["M"], None, proj["bias"], out=y)
        return y

    def forward(self, x: torch.Tensor):
        """x [N, C, T] -> [N, C, T]."""
        hip.require_device(x, "SingleRNN.forward")
        t = x.shape[-1]
        return hip.unpad_rows(self.forward_padded(hip.pad_rows(x), t), t)
