"""CPU tests of the inference forward's plan (skoots_amd/plan.py) and of what ``HipUNet.forward_tiles`` launches from it.

``test_launch_trace_*``: the forward runs on the CPU under the recorder of tests/golden/make_forward_trace_golden.py and
must issue, call for call, what tests/golden/forward_trace.json holds -- the same library functions with the same
scalars on the same named buffers in the same order; with deterministic kernels that is the same output, bit for bit.
The other tests work on ``plan_forward`` alone: no tensor, no library call."""
import importlib.util
import itertools
import json
import os

import pytest

from skoots_amd.plan import PRECISIONS, Form, Kernel, conv_flops, network_blocks, plan_forward

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NETWORKS = (((32, 64, 128, 64, 32), (2, 2, 2, 2, 2)), ((32, 32, 64, 32, 32), (1, 2, 3, 2, 1)),
            ((32, 64, 64, 64, 32), (3, 1, 1, 1, 3)))
BOOLS = (True, False)
# (network, precision, defer_activation, fold_upsample, box_store, stem_single_pass, keep_features, has_box, fold_ok)
PLAN_INPUTS = [(*net, prec, *flags, (f0, f1)) for net in NETWORKS for prec in ("fp16", "split", "mix8")
               for flags in itertools.product(BOOLS, repeat=6) for f0 in BOOLS for f1 in BOOLS]
MIX8_KERNELS, FOLDED = (Kernel.MIX8, Kernel.UPFOLD_MIX8), (Kernel.UPFOLD, Kernel.UPFOLD_MIX8)


# ---- A. the launch trace ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def traces():
    spec = importlib.util.spec_from_file_location("make_forward_trace_golden",
                                                  os.path.join(GOLDEN, "make_forward_trace_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(GOLDEN, "forward_trace.json")) as f:
        want = json.load(f)
    return want, json.loads(json.dumps(gen.record_all()))


def _expanded(doc, key):
    t = dict(doc["traces"][doc["configurations"][key]])
    t["calls"] = [doc["calls"][i] for i in t["calls"]]
    return t


def test_launch_trace_covers_the_configurations(traces):
    want, got = traces
    assert list(got["configurations"]) == list(want["configurations"]) and len(want["configurations"]) >= 576 + 6
    kernels = {want["calls"][i][0] for t in want["traces"] for i in t["calls"]}
    assert {"sk_conv3d", "sk_conv3d_split", "sk_conv3d_mix8", "sk_conv3d_box", "sk_conv3d_box_split", "sk_conv3d_upfold",
            "sk_conv3d_upfold_split", "sk_conv3d_upfold_mix8", "sk_conv3d_down_act", "sk_conv3d_down_act_split",
            "sk_conv3d_down_act_mix8", "sk_conv3d_stem", "sk_conv3d_stem_raw", "sk_conv3d_stem_apply",
            "sk_conv3d_stem_apply_split", "sk_conv3d_stem_apply_mix8", "sk_groupnorm_finalize", "sk_groupnorm_silu",
            "sk_groupnorm_silu_split", "sk_groupnorm_silu_mix8", "sk_groupnorm_silu_f32", "sk_conv3d_f32", "sk_heads",
            "sk_heads_split"} <= kernels


def test_launch_trace_equals_the_fixture(traces):
    """Call for call; with the ConvProfile's executed FLOPs and (flops, name) events, the output's shape and the
    names in ``last_features``."""
    want, got = traces
    for key in want["configurations"]:
        w, g = _expanded(want, key), _expanded(got, key)
        for i, (a, b) in enumerate(zip(w["calls"], g["calls"])):
            assert a == b, f"{key}: call {i}"
        assert g == w, key


def test_random_state_dict_is_unchanged(traces):
    want, got = traces
    assert got["state_dict_sha256"] == want["state_dict_sha256"]


# ---- B. properties of the plan ----------------------------------------------------------------------------------------------
def _table(plan):
    """(name, family, what it leaves or writes back) per step, as readable strings."""
    return [(s.name, s.kernel.value + (" box" if s.box and s.kernel is Kernel.MIX8 else ""), (s.writeback or s.out).value) for s in plan]


def test_default_network_mix8_with_out_box():
    plan = plan_forward((32, 64, 128, 64, 32), (2, 2, 2, 2, 2), "mix8", has_box=True)
    assert _table(plan) == [
        ("enc0.0", "stem", "mix8"),               # two passes, the second stores mix8 lines
        ("enc0.1", "mix8", "raw"),                # the skip tensor: activated by down0
        ("down0", "down act", "mix8"),            # writes skip0 back as mix8 lines for dec0.0
        ("enc1.0", "mix8", "mix8"),
        ("enc1.1", "mix8", "raw"),
        ("down1", "down act", "mix8"),
        ("mid.0", "mix8", "mix8"),
        ("mid.1", "mix8", "raw"),                 # red1 activates it on load
        ("red1", "conv", "mix8"),                 # split 1x1x1
        ("dec1.0", "upfold mix8", "mix8"),
        ("dec1.1", "mix8", "raw"),
        ("red0", "conv", "mix8"),
        ("dec0.0", "upfold mix8", "mix8"),
        ("dec0.1", "mix8 box", "raw"),            # the heads read only the box
        ("heads", "heads", "fp16")]
    assert all(s.store is Form.SPLIT for s in plan)
    assert [s.norm_pass for s in plan if s.name in ("enc0.0", "down0", "red1", "dec0.1")] == [None, Form.MIX8, Form.MIX8, None]
    assert [(s.tag, [x.tag for x in s.srcs]) for s in plan] == [
        ("L0a", ["image"]), ("skip0", ["L0a"]), ("L1a", ["skip0"]), ("L1b", ["L1a"]), ("skip1", ["L1b"]),
        ("L2a", ["skip1"]), ("L2b", ["L2a"]), ("L2a", ["L2b"]), ("L2r", ["L2a"]), ("L1a", ["skip1", "L2r"]),
        ("L1b", ["L1a"]), ("L1r", ["L1b"]), ("L0a", ["skip0", "L1r"]), ("L0b", ["L0a"]), ("out5", ["L0b"])]


def test_default_network_fp16():
    """The fast path: every activation that was measured to pay is fused into its reader."""
    plan = plan_forward((32, 64, 128, 64, 32), (2, 2, 2, 2, 2), "fp16", has_box=True)
    assert _table(plan) == [
        ("enc0.0", "stem", "fp16"), ("enc0.1", "conv", "raw"), ("down0", "down act", "fp16"), ("enc1.0", "conv", "fp16"),
        ("enc1.1", "conv", "raw"), ("down1", "down act", "fp16"), ("mid.0", "conv", "fp16"), ("mid.1", "conv", "raw"),
        ("red1", "conv", "fp16"), ("dec1.0", "upfold", "fp16"), ("dec1.1", "conv", "raw"), ("red0", "conv", "fp16"),
        ("dec0.0", "upfold", "raw"), ("dec0.1", "conv box", "raw"), ("heads", "heads", "fp16")]
    single = plan_forward((32, 64, 128, 64, 32), (2, 2, 2, 2, 2), "fp16", stem_single_pass=True)
    assert _table(single)[:2] == [("enc0.0", "stem raw", "raw"), ("enc0.1", "conv", "raw")]


def test_network_blocks_is_the_unet():
    blocks = network_blocks((32, 64, 128, 64, 32), (2, 1, 2, 2, 1))
    assert [(b.name, b.ksize, b.cin, b.cout, b.level) for b in blocks] == [
        ("enc0.0", 3, 1, 32, 0), ("enc0.1", 3, 32, 32, 0), ("down0", 2, 32, 64, 1), ("enc1.0", 3, 64, 64, 1),
        ("down1", 2, 64, 128, 2), ("mid.0", 3, 128, 128, 2), ("mid.1", 3, 128, 128, 2), ("red1", 1, 128, 64, 2),
        ("dec1.0", 3, 128, 64, 1), ("dec1.1", 3, 64, 64, 1), ("red0", 1, 64, 32, 1), ("dec0.0", 3, 64, 32, 0)]
    assert blocks[8].srcs == (("enc1.0", 0, 64), ("red1", 1, 64)) and blocks[-1].srcs == (("enc0.1", 0, 32), ("red0", 1, 32))
    assert blocks[0].srcs == (("image", 0, 1),)


@pytest.mark.parametrize("precision", ["fp16", "split", "mix8"])
def test_sources_are_read_in_a_form_the_kernel_accepts(precision):
    for args in (a for a in PLAN_INPUTS if a[2] == precision):
        for s in plan_forward(*args):
            forms = [x.form for x in s.srcs]
            if s.kernel in MIX8_KERNELS:     # mix8 lines only: one C -> C source, or a folded pair
                assert all(f is Form.MIX8 for f in forms), (args, s)
                assert [x.up for x in s.srcs] == ([0, 1] if s.kernel is Kernel.UPFOLD_MIX8 else [0]), (args, s)
                assert s.ksize == 3 and (s.kernel is Kernel.UPFOLD_MIX8 or s.srcs[0].c == s.cout), (args, s)
            else:
                assert Form.MIX8 not in forms, (args, s)
            if s.kernel is Kernel.UPFOLD:    # two activated sources, the second upsampled
                assert forms == [s.store, s.store] and [x.up for x in s.srcs] == [0, 1], (args, s)
            if s.kernel in FOLDED:
                assert args[4] and args[-1][s.level], (args, s)   # fold_upsample, and the kernel covers the shape
            for x in s.srcs:
                if x.form is Form.RAW:
                    assert (s.kernel in (Kernel.DOWN_ACT, Kernel.HEADS) or (s.kernel is Kernel.CONV and s.ksize == 1) or
                            (s.kernel in (Kernel.CONV, Kernel.CONV_BOX) and s.ksize == 3 and precision == "fp16" and
                             x.c == 32 and len(s.srcs) == 1)), (args, s)
                    assert not x.up, (args, s)
                elif x.name != "image":
                    assert x.form in (s.store, Form.MIX8), (args, s)


def test_no_step_overwrites_a_tensor_that_is_still_read():
    for args in PLAN_INPUTS:
        plan = plan_forward(*args)
        index = {s.name: i for i, s in enumerate(plan)}
        for j, s in enumerate(plan):
            for x in s.srcs:
                first = index.get(x.name, -1) + 1     # "image" is nobody's output
                assert x.tag == (plan[first - 1].tag if first else "image"), (args, s)
                assert all(w.tag != x.tag for w in plan[first:j + 1]), (args, s)


def test_raw_skip_is_written_back_in_the_form_the_decoder_reads():
    seen = set()
    for args in PLAN_INPUTS:
        plan = plan_forward(*args)
        by_name = {s.name: s for s in plan}
        for i, s in enumerate(plan):
            if s.ksize != 2:
                assert s.writeback is None, (args, s)
                continue
            skip = by_name[s.srcs[0].name]
            assert (s.kernel is Kernel.DOWN_ACT) == (skip.out is Form.RAW), (args, s)
            (j, decoder), = [(j, d) for j, d in enumerate(plan) if d is not s and any(x.name == skip.name for x in d.srcs)]
            assert j > i and decoder.srcs[0].name == skip.name, (args, s)
            if s.kernel is Kernel.DOWN_ACT:
                assert s.writeback in (s.store, Form.MIX8) and decoder.srcs[0].form is s.writeback, (args, s)
                assert (s.writeback is Form.MIX8) == (decoder.kernel is Kernel.UPFOLD_MIX8), (args, s)
            else:
                assert s.kernel is Kernel.DOWN and decoder.srcs[0].form is skip.out is s.store, (args, s)
            seen.add((s.kernel, s.writeback))
    assert seen == {(Kernel.DOWN, None), (Kernel.DOWN_ACT, Form.F16), (Kernel.DOWN_ACT, Form.SPLIT), (Kernel.DOWN_ACT, Form.MIX8)}


def test_keep_features_leaves_plain_activated_tensors():
    for args in PLAN_INPUTS:
        plan, keep = plan_forward(*args), args[7]
        assert all(s.keep == keep for s in plan[:-1]) and not plan[-1].keep
        if keep:
            assert all(s.out is s.store for s in plan[:-2]), args          # no RAW, no mix8 lines
            assert plan[-2].out is (Form.RAW if args[3] else plan[-2].store), args   # as ever: the heads' input stays RAW
            assert not any(s.kernel in MIX8_KERNELS + (Kernel.DOWN_ACT, Kernel.STEM_RAW) for s in plan), args


def test_store_box_only_on_the_last_conv():
    boxed = 0
    for args in PLAN_INPUTS:
        plan = plan_forward(*args)
        defer, box_store, keep, has_box = args[3], args[5], args[7], args[8]
        assert not any(s.box for s in plan[:-2]) and not plan[-1].box, args
        last = plan[-2]
        assert last.name.startswith("dec0.") and (last.kernel is Kernel.CONV_BOX) <= last.box
        if last.box:
            assert last.out is Form.RAW and has_box and box_store and defer and not keep, args
            assert last.kernel in (Kernel.CONV_BOX, Kernel.MIX8), args
            boxed += 1
        elif has_box and box_store and defer and not keep:   # the folded kernels have no box variant
            assert last.kernel in FOLDED, args
    assert boxed


def test_fp32_plan_runs_every_block_on_the_fp32_kernels():
    plan = plan_forward((32, 64, 128, 64, 32), (2, 2, 2, 2, 2), "fp32", keep_features=True, has_box=True)
    assert [s.kernel for s in plan] == [Kernel.F32] * 14 + [Kernel.HEADS_F32]
    assert all(s.out is Form.F32 and not s.box and not s.keep for s in plan)


def test_conv_flops_by_family():
    plan = {s.name: s for s in plan_forward((32, 64, 128, 64, 32), (2, 2, 2, 2, 2), "mix8")}
    k128 = 1.0 + 10.0 / 9.0
    assert conv_flops(plan["enc0.1"]) == (2.0 * 32 * 32 * 27, 2.0 * 32 * 32 * 27, k128)
    assert conv_flops(plan["mid.0"]) == (2.0 * 128 * 128 * 27, 2.0 * 128 * 128 * 27, 2.0)
    assert conv_flops(plan["dec0.0"]) == (2.0 * 64 * 32 * 27, 2.0 * 32 * (32 * 27 * k128 + 32 * 8 * 2.0), 1.0)
    split = {s.name: s for s in plan_forward((32, 64, 128, 64, 32), (2, 2, 2, 2, 2), "split")}
    assert conv_flops(split["dec1.0"]) == (2.0 * 128 * 64 * 27, 2.0 * 64 * (64 * 27 + 64 * 8), 3.0)
    assert conv_flops(split["enc1.0"]) == (2.0 * 64 * 64 * 27, 2.0 * 64 * 64 * 27, 3.0)


def test_planner_errors():
    with pytest.raises(ValueError, match="precision must be one of"):
        plan_forward((32, 64, 128, 64, 32), (2, 2, 2, 2, 2), "bf16")
    with pytest.raises(ValueError, match="unsupported dims .*: kernels are built for widths 32/64/128"):
        plan_forward((32, 48, 128, 48, 32), (2, 2, 2, 2, 2), "fp16")
    assert PRECISIONS == ("fp16", "split", "mix8", "fp32")


# ---- stream contexts -------------------------------------------------------------------------------------------------
def test_stream_context_reads_its_models_switches():
    from skoots_amd import unet
    model = unet.HipUNet(unet.random_state_dict(), "cpu")
    ctx = model.clone_context()
    assert ctx.layers is model.layers and ctx._bufs is not model._bufs
    for name, value in (("precision", "mix8"), ("defer_activation", False), ("fold_upsample", False), ("box_store", False),
                        ("stem_single_pass", True)):
        assert getattr(ctx, name) == getattr(model, name) != value
        setattr(model, name, value)
        assert getattr(ctx, name) == getattr(model, name) == value
    assert model.clone_context().stem_single_pass is True
    with pytest.raises(ValueError, match="precision must be one of"):
        unet.HipUNet(unet.random_state_dict(), "cpu", precision="bf16")
