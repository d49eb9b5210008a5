"""Captured graphs against later calls on the same model: the schedules, shapes and the kept-rows arithmetic shared by
test_h_rows.py (CPU) and test_graph_interleave_gpu.py.  Needs no GPU and no library.

A captured graph holds raw addresses of what the model keeps from call to call: packed-weight plans, the kept scratch of
PlanCache and the zeroed LSTM output rows of _plans._h_rows.  Every other replay test captures and replays with nothing in
between; here another length, another batch, an eager call, another capture and freed memory full of NaN come between a
capture and its replay.

Presets, weights, inputs, length_of and the two arithmetics are edge_length_cases'.  Three frame counts per preset:
  a = 3     a short utterance;
  b = 127   the same 128-frame row as `a`, so the two share every buffer shape and differ in the LSTM walks: frames `b`
            writes are pad frames of `a`, and they outnumber a's own 42 to 1;
  c = 129   the next row length: buffers are replaced, workspaces grow.
The batch is 2, and `b` also runs at a batch of 1.  These are the smallest shapes at which one row holds two geometries
and a third shape replaces the buffers.  A step's input is rows [i, i + B) of the preset's deterministic mixture, i the
step's index: no two steps of a schedule see the same samples, so a replay that did nothing cannot pass on what an earlier
step left in the graph's static output."""
import edge_length_cases as E

PRESETS = E.PRESETS
PRECISIONS = E.PRECISIONS
BATCH = 2
FRAMES = {"a": 3, "b": 127, "c": 129}
#: shape name -> (frame count, batch)
SHAPES = {"a": (FRAMES["a"], BATCH), "b": (FRAMES["b"], BATCH), "c": (FRAMES["c"], BATCH), "b1": (FRAMES["b"], 1)}

# Part A.  ("graph" | "eager" | "churn", shape name, whether the kept-rows check follows): "graph" is
# GraphedInference(served)(x) -- a capture at a shape's first use, a replay afterwards --, "eager" is served.inference(x),
# "churn" fills the caching allocator with NaN.  Every graph / eager step is compared with plain.inference(x).
PART_A = (
    ("graph", "a", False),     # 1. capture short,
    ("graph", "b", False),     #    capture long in the same row,
    ("graph", "a", True),      #    replay short behind it: its pad frames must not hold the long call's rows
    ("eager", "c", False),     # 2. another row length on the served model: buffers replaced, workspaces grown
    ("churn", None, False),
    ("graph", "b", True),
    ("graph", "a", True),
    ("graph", "b1", True),     #    (a capture at another batch)
    ("graph", "b", True),
    ("eager", "a", False),     # 3. eagerly, directly behind a replay of the long graph: no host record knows of that replay
    ("graph", "a", False),     # 4.
)


def step_input(name, shape, step):
    """-> (mixture [B, L], enrolment [B, L_ENROLL] or None) of step number `step` of a schedule at `shape`"""
    t, batch = SHAPES[shape]
    noisy, enroll = E.inputs(name, E.length_of(name, t), batch + step)
    return noisy[step:].clone(), (None if enroll is None else enroll[step:].clone())


def describe(i):
    kind, shape, _ = PART_A[i]
    if kind == "churn":
        return f"step {i}: NaN through the allocator"
    t, batch = SHAPES[shape]
    return f"step {i}: {kind} call at T = {t}, B = {batch} (after {[k + ' ' + (s or '') for k, s, _ in PART_A[:i]]})"


# ---------------------------------------------------------------------------------------------------------------------
# kept rows
# ---------------------------------------------------------------------------------------------------------------------
def written_frames(walk):
    """The frames of a row a recurrence writes on the walk (q, q_stride, steps, step_stride): sequence s, step k ->
    frame s * q_stride + k * step_stride."""
    q, q_stride, steps, step_stride = walk
    return sorted({s * q_stride + k * step_stride for s in range(q) for k in range(steps)})


def pad_frames_are_zero(buf, walk):
    """Whether every frame of buf [N, rows, ldt] outside written_frames(walk) is exactly 0.0 -> (bool, number of
    non-zero pad values)."""
    import torch
    pad = torch.ones(buf.shape[-1], dtype=torch.bool, device=buf.device)
    pad[torch.tensor(written_frames(walk), device=buf.device)] = False
    bad = int(torch.count_nonzero(buf[..., pad] != 0.0))    # (NaN != 0.0 too)
    return bad == 0, bad


def kept_rows(obj, out=None):
    """Every buffer _plans._h_rows keeps under `obj` (a plan: nested dicts / lists / tuples) -> [(lane, geometry =
    (t, q, q_stride, steps, step_stride), buffer)]."""
    out = [] if out is None else out
    if isinstance(obj, dict):
        for k, v in obj.items():
            if k == "h_rows":
                for lane, bufs in v.items():
                    for (_, _, geometry), buf in bufs.items():
                        out.append((lane, geometry, buf))
            else:
                kept_rows(v, out)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            kept_rows(v, out)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Part B: a streaming session while its model serves other calls
# ---------------------------------------------------------------------------------------------------------------------
#: streamer class -> the preset its own GPU test file streams
STREAMERS = (("StreamingSeparator", "ns_dpcrn_short"), ("StreamingSeparator", "ns_dparn_short"),
             ("StreamingConvTasNet", "cfg3_causal_short"), ("StreamingDPRNN", "cfg4_tse_short"),
             ("StreamingSkiMExtractor", "tse_skim_causal_short"), ("StreamingUnetTcn", "tse_unet_tcn_causal_short"))
STREAMS = 3            # B of the session under test
HOPS = 40              # hops of the stream (priming included), fed in chunks of CHUNK_HOPS
CHUNK_HOPS = 4
OTHER_STREAMS = 2      # B of the second session
OTHER_HOPS = 12        # hops the second session is stepped: past the priming and the model delay of every preset
#: the offline calls between the thirds of the stream: (frames, batch), a larger shape first, then a smaller one
OFFLINE = ((129, 4), (3, 1))


def thirds(n_chunks):
    """Chunk indices behind which the disturbance is inserted: after each third of the stream."""
    return (n_chunks // 3, 2 * n_chunks // 3)
