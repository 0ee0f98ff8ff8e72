"""Every switch of the engine's table (aldi_amd/engine.py: EngineKnobs) against the default table on one small bf16 model: the other arm is
reached (another sequence of native calls / streams, or the state that tells the two arms apart) and the whole gradient buffer agrees with the
default's within the bound measured for that switch (twice the measured delta; no delta measured: bit for bit)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
K, H, W = 8, 192, 256             # every pyramid level halves exactly (the upsample chain is eligible); three stride-2 stage entrances
SCALES = {"loss_cls": 1.0, "loss_box_reg": 1.0, "loss_rpn_cls": 1.0, "loss_rpn_loc": 1.0}
STREAM_SWITCHES = ("aux_stream", "wgrad_stream", "wgrad_prio")      # read when a side stream is created: the streams are dropped around their cases

# switch: (other arm, "forward": a whole forward + backward under it | "backward": the backward again on the default run's context,
#          the (entry point, on the default stream) sequence differs from the default's, bound on max|d grad| / max|grad|: 0 = torch.equal)
SWITCHES = {
    "fused_stem": (False, "forward", True, 0),
    "fused_res2": (False, "forward", True, 2 * 1.1789e-02),
    "fused_res2_shortcut": (False, "forward", True, 0),
    "fused_stage_entrance": (False, "forward", True, 0),
    "level_groups": (False, "forward", True, 0),
    "mask_bits": (False, "forward", False, 0),
    "mask_bits_inner": (False, "forward", False, 0),
    "mask_bits_fc": (False, "forward", False, 0),
    "roi_prepare_fused": (False, "forward", True, 0),
    "box_loss_fused": (False, "backward", True, 0),
    "sparse_rpn_backward": (False, "backward", True, 2 * 3.0216e-04),
    "upsample_chain": (False, "backward", True, 0),
    "aux_stream": (False, "backward", True, 0),
    "wgrad_stream": (False, "backward", True, 0),
    "wgrad_prio": (-1, "backward", False, 0),
    "group_wgrad": (False, "backward", True, 2 * 1.8147e-07),
    "wgrad_tail_split": (0, "backward", True, 0),
    "wgrad_subsample": (False, "backward", True, 2 * 5.4441e-08),
    "wgrad_subsample_side": (False, "backward", True, 0),
    "wgrad_bias_fused": (False, "backward", True, 2 * 1.8147e-08),
}


def _bits(c):
    """which saved activations have a ReLU bit mask beside them: (block outputs, inner maps, FC2)"""
    ob = c.get("out_bits") or {}
    has = lambda t: t.data_ptr() in ob
    return (sum(has(blk[4]) for blk in c.blocks), sum(has(blk[2]) + has(blk[3]) for blk in c.blocks), has(c.fc2))


# the switches that change operands only: what tells the arm from the default after the run
STATE = {
    "mask_bits": lambda m, c: _bits(c) == (0, 0, False),
    "mask_bits_inner": lambda m, c: _bits(c) == (13, 0, True),
    "mask_bits_fc": lambda m, c: _bits(c) == (13, 26, False),
    "wgrad_prio": lambda m, c: m._wg_side.priority == -1,
}


class _Recorder:
    """(entry point, on the default stream) of every native call made through _lib.call while it is installed"""

    def __enter__(self):
        from aldi_amd import _lib as L
        self.seq, self.lib, self.orig = [], L, L.call

        def call(name, *args):
            self.seq.append((name, torch.cuda.current_stream() == torch.cuda.default_stream()))
            return self.orig(name, *args)
        L.call = call
        return self.seq

    def __exit__(self, *exc):
        self.lib.call = self.orig
        return False


def _drop_streams(m):
    m.__dict__.pop("_wg_side", None)
    m.__dict__.pop("_aux_side", None)


def _forward(m, data):
    torch.manual_seed(5)
    return m.forward_train([d["image"] for d in data], [d["instances"] for d in data], roi_seed=9)


def _backward(m, wts, c):
    wts.zero_grad()
    m.backward(c, SCALES)
    torch.cuda.synchronize()
    assert int(m.err) == 0
    return wts.grad.clone()


@pytest.fixture(scope="module")
def default():
    """the model, and the default table's run: context, gradient, and the call sequences of its forward and its backward"""
    from aldi_amd import synthetic as syn
    from aldi_amd.arch import ParamLayout
    from aldi_amd.engine import RCNN, EngineKnobs, Weights
    wts = Weights(ParamLayout(K), torch.device(DEV), torch.bfloat16, trainable=True)
    wts.load_state_dict(syn.init_state_dict(K, seed=1))
    m = RCNN(wts, K, knobs=EngineKnobs.from_env(env={}))
    # (behind the engine's constructor, which leaves torch with one CPU thread: the synthetic images depend on the thread count they are
    # drawn with, and the bounds above were measured on these)
    _, data, _, _ = syn.make_batch(2, 0, H, W, K, seed=0, boxes_per_image=(3, 6))
    _backward(m, wts, _forward(m, data))          # (first use: dgrad weights are derived layer by layer, plans are built)
    with _Recorder() as fwd:
        c = _forward(m, data)
    with _Recorder() as bwd:
        grad = _backward(m, wts, c)
    assert c.R > 0 and _bits(c) == (13, 26, True) and float(grad.abs().max()) > 0
    assert m._wg_side is not None and m._wg_side.priority == 0 and m._aux_side is not None
    return m, wts, data, c, grad, list(fwd), list(bwd)


def test_default_run_repeats_itself(default):
    """the reference of every case below: a second default run makes the same calls and gives the same gradient"""
    m, wts, data, c0, grad0, fwd0, bwd0 = default
    with _Recorder() as seq:
        grad = _backward(m, wts, _forward(m, data))
    assert seq == fwd0 + bwd0
    assert torch.equal(grad, grad0)


def test_the_table_of_cases_covers_every_switch():
    import dataclasses
    from aldi_amd.engine import EngineKnobs
    assert set(SWITCHES) == {f.name for f in dataclasses.fields(EngineKnobs)}
    assert all(getattr(EngineKnobs(), name) != SWITCHES[name][0] for name in SWITCHES)
    assert {name for name in SWITCHES if not SWITCHES[name][2]} == set(STATE)


@pytest.mark.parametrize("name", sorted(SWITCHES))
def test_switch_reaches_its_other_arm_and_keeps_the_gradient(default, name):
    m, wts, data, c0, grad0, fwd0, bwd0 = default
    value, where, seq_differs, bound = SWITCHES[name]
    old = m.knobs
    if name in STREAM_SWITCHES:
        _drop_streams(m)
    try:
        with m.with_knobs(**{name: value}):
            for _ in range(2):                    # (the first pass derives what the arm uses for the first time; the second one is compared)
                with _Recorder() as seq:
                    c = _forward(m, data) if where == "forward" else c0
                    grad = _backward(m, wts, c)
            told_apart = STATE[name](m, c) if name in STATE else None
    finally:
        if name in STREAM_SWITCHES:
            _drop_streams(m)
    assert m.knobs is old
    assert (seq != (fwd0 + bwd0 if where == "forward" else bwd0)) == seq_differs
    if name in STATE:
        assert told_apart
    delta, top = float((grad - grad0).abs().max()), float(grad0.abs().max())
    print(f"{name}: max|d grad| / max|grad| = {delta / top:.4e} (bound {bound:.4e}; max|grad| {top:.9g})")
    if bound == 0:
        assert torch.equal(grad, grad0)
    else:
        assert delta <= bound * top
