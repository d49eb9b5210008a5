"""The shared batch of the ragged SkiM tests (test_ragged_skim.py, test_ragged_skim_gpu.py): edge_length_cases' utterances at
the frame counts where a length turns into another segment count of SkiM(seg_size=150), each followed by junk, and per row
the float64 oracle of the utterance alone (ragged_ref.batch: computed once, shared, never written to).

SKIM_T: one frame; both sides of a segment boundary (149 | 150 | 151, 300 | 301); T_n % K == 0 (150, 300, 450: the utterance
alone then carries a whole segment of zeros); S_n = T_n // K + 1 from 1 to S = 4 of the 451-frame row."""
import torch

import cases
import edge_length_cases as E
import ragged_ref as R
from oracle import separator_oracle as O

NAMES = ("tse_skim_causal_short", "tse_skim_v0_short", "tse_skim_vad_short", "tse_skim_v1_short")
SKIM_T = (451, 1, 149, 150, 151, 300, 301, 450)
SKIM_ENROL_T = (186, 1, 2, 128, 129, 186, 50, 186)
SEG = 150
SEG_ROWS = [t // SEG + 1 for t in SKIM_T]
EQUAL_T = (151, 151, 151)     # three rows of one length: where the causal hand-over between utterances shows
EQUAL_ENROL_T = (186, 186, 186)


def batch(name, junk="noise"):
    """-> (noisy [8, L], lengths, enroll [8, L'], enroll_lengths, refs) of ragged_ref.batch"""
    return R.batch(name, SKIM_T, SKIM_ENROL_T, junk)


def equal_batch(name):
    return R.batch(name, EQUAL_T, EQUAL_ENROL_T)


def oracle_padded(name, noisy, lens, enroll, e_lens):
    """The float64 oracle of the batch with zeros for junk: what zero-padding computes"""
    x = torch.zeros_like(noisy, dtype=torch.float64)
    e = torch.zeros_like(enroll, dtype=torch.float64)
    for n, (a, b) in enumerate(zip(lens, e_lens)):
        x[n, :a] = noisy[n, :a].double()
        e[n, :b] = enroll[n, :b].double()
    with torch.no_grad():
        return O.inference(x, E.weights(name)[1], cases.oracle_cfg(name), e)
