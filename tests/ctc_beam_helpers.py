"""What tests/test_ctc_beam.py and tests/test_ctc_word_beam.py share: the layouts the searches are fed in, reading the strings out of a result,
and small input builders.  No oracle code lives here -- the two oracles stay separate and share nothing with the kernels."""
import numpy as np
import torch


def layout(dev, utts, layout='packed', ld=None, gaps=None):
    """utts: list of (T_i, V) float32 arrays.  layout 'packed': back to back, or with gaps[i] NaN rows in front of utterance i; 'slots': slot b
    starts at b * T_max, NaN filler.  ld > V: NaN in the extra columns.  Returns the leading arguments of both search ops: the logits matrix
    and the (first frame, frames) table on dev, then V, the frames in all and the longest utterance (at least 1)."""
    V = utts[0].shape[1]
    ld = ld or V
    frames = [int(x.shape[0]) for x in utts]
    if layout == 'slots':
        first = [b * max(frames) for b in range(len(utts))]
        rows = len(utts) * max(frames)
    else:
        gaps = gaps or [0] * len(utts)
        first, at = [], 0
        for g, n in zip(gaps, frames):
            first.append(at + g)
            at += g + n
        rows = at
    flat = np.full((rows, ld), np.nan, dtype=np.float32)
    for f0, x in zip(first, utts):
        flat[f0:f0 + x.shape[0], :V] = x
    utt = torch.tensor([[f, n] for f, n in zip(first, frames)], dtype=torch.int64).reshape(len(utts), 2).to(dev)
    return torch.from_numpy(flat).to(dev), utt, V, sum(frames), max(max(frames), 1)


def strings(out, b):
    labels, lengths = out[0], out[1]
    return [tuple(labels[b, r, :lengths[b, r]].tolist()) for r in range(lengths.shape[1]) if lengths[b, r] >= 0]


def noise(rng, T, V, blank, s):
    x = rng.standard_normal((T, V)) * s
    x[:, blank] += s
    return x.astype(np.float32)


def from_probs(rows):
    return np.log(np.asarray(rows, dtype=np.float64)).astype(np.float32)


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=False) for x, y in zip(a, b))
