"""CPU tests of the training backward's gradient routing (skoots_amd/train/routes.py): ``route_gradients`` on graphs
described with integer keys.  No tensor and no kernel is involved: which way each data gradient travels is a function
of the recorded graph and ``f16_grad_handoff`` alone."""
import pytest

from skoots_amd.train import engine as E

Kind, Route, GraphBlock = E.Kind, E.Route, E.GraphBlock
IMAGE = 0
COMPLETE_16 = (Route.DIRECT, Route.INTERLEAVED, Route.POOLED, Route.HEADS)


def _unet(dims=(32, 64, 128, 64, 32), fast=True, heads16=True):
    """The graph ``TrainUNet.forward`` records with depths (2, 2, 2, 2, 2): 14 GroupNorm blocks, then the heads."""
    d0, d1, d2, d3, d4 = dims
    norm = Kind.FAST if fast else Kind.FP32
    blocks = []

    def add(name, kind, ksize, cout, *srcs):
        blocks.append(GraphBlock(name, kind, ksize, cout, len(blocks) + 1, srcs))
        return len(blocks)

    a = add("enc0.0", Kind.STEM if fast else Kind.FP32, 3, d0, (IMAGE, 0, 1))
    s0 = add("enc0.1", norm, 3, d0, (a, 0, d0))
    a = add("down0", norm, 2, d1, (s0, 0, d0))
    a = add("enc1.0", norm, 3, d1, (a, 0, d1))
    s1 = add("enc1.1", norm, 3, d1, (a, 0, d1))
    a = add("down1", norm, 2, d2, (s1, 0, d1))
    a = add("mid.0", norm, 3, d2, (a, 0, d2))
    a = add("mid.1", norm, 3, d2, (a, 0, d2))
    r1 = add("red1", norm, 1, d3, (a, 0, d2))
    a = add("dec1.0", norm, 3, d3, (s1, 0, d1), (r1, 1, d3))
    a = add("dec1.1", norm, 3, d3, (a, 0, d3))
    r0 = add("red0", norm, 1, d4, (a, 0, d3))
    a = add("dec0.0", norm, 3, d4, (s0, 0, d0), (r0, 1, d4))
    a = add("dec0.1", norm, 3, d4, (a, 0, d4))
    add("heads", Kind.HEADS16 if fast and heads16 else Kind.FP32, 1, 5, (a, 0, d4))
    return blocks


def _by_name(graph, handoff):
    return {b.name: r for b, r in zip(graph, E.route_gradients(graph, IMAGE, handoff))}


GRAPHS = {"default": (_unet(), True), "handoff_off": (_unet(), False), "all_fp32": (_unet(fast=False), True),
          "all_fp32_handoff_off": (_unet(fast=False), False),
          "last_width_64": (_unet(dims=(32, 64, 128, 64, 64), heads16=False), True)}


def test_default_network_with_handoff():
    """The 16-bit step of the default network: no fp32 gradient tensor exists besides dlogits."""
    D, P, I, L, H, N = Route.DIRECT, Route.PENDING, Route.INTERLEAVED, Route.POOLED, Route.HEADS, Route.NONE
    assert _by_name(*GRAPHS["default"]) == {
        "heads": [H],                    # dec0.1's output: from the heads
        "dec0.1": [D], "red0": [D], "dec1.1": [D], "red1": [D], "mid.1": [D], "mid.0": [D], "enc1.1": [D],
        "enc1.0": [D], "enc0.1": [D],    # the outputs of dec0.0, dec1.1, dec1.0, mid.1, mid.0, down1, enc1.0, down0, enc0.0
        "dec0.0": [P, L], "dec1.0": [P, L],   # the skips wait for their stride-2 reader; red0 / red1 pooled
        "down0": [I], "down1": [I],      # the skips' sums, inside the interleave
        "enc0.0": [N]}                   # the image


def test_handoff_off_is_all_fp32():
    routes = _by_name(*GRAPHS["handoff_off"])
    assert routes.pop("enc0.0") == [Route.NONE]
    assert all(r is Route.FP32 for rs in routes.values() for r in rs) and len(routes) == 14


@pytest.mark.parametrize("handoff", [True, False])
def test_fp32_blocks_are_all_fp32(handoff):
    routes = _by_name(_unet(fast=False), handoff)
    assert routes.pop("enc0.0") == [Route.NONE]
    assert all(r is Route.FP32 for rs in routes.values() for r in rs) and len(routes) == 14


def test_fp32_heads_behind_a_16bit_block():
    """Last width 64: the heads are not the 32 -> 5 kernel, so they run as an fp32 block on dec0.1's fp32 copy and
    hand an fp32 gradient to a fast block; everything upstream is as in the default network."""
    routes = _by_name(*GRAPHS["last_width_64"])
    assert routes["heads"] == [Route.FP32]
    want = _by_name(*GRAPHS["default"])
    assert {k: v for k, v in routes.items() if k != "heads"} == {k: v for k, v in want.items() if k != "heads"}


@pytest.mark.parametrize("which", sorted(GRAPHS))
def test_every_gradient_is_delivered_once(which):
    graph, handoff = GRAPHS[which]
    routes = E.route_gradients(graph, IMAGE, handoff)
    assert [len(r) for r in routes] == [len(b.srcs) for b in graph]
    producer = {b.out: i for i, b in enumerate(graph)}
    got = {}                                   # key -> routes in the order the backward delivers them
    for i in reversed(range(len(graph))):
        for (key, _, _), route in zip(graph[i].srcs, routes[i]):
            assert (route is Route.NONE) == (key == IMAGE)
            if key != IMAGE:
                assert producer[key] < i       # delivered before the producer's block is walked
                got.setdefault(key, []).append(route)
    assert set(got) == set(producer) - {graph[-1].out}
    for key, rs in got.items():
        if rs[0] is Route.PENDING:             # followed by exactly one summing route
            assert rs == [Route.PENDING, Route.INTERLEAVED], (key, rs)
        elif rs[0] in COMPLETE_16:             # one complete 16-bit delivery, nothing else
            assert len(rs) == 1, (key, rs)
        else:                                  # one fp32 tensor: created, then accumulated
            assert all(r is Route.FP32 for r in rs), (key, rs)


@pytest.mark.parametrize("fast", [True, False])
def test_upsampled_tensor_read_twice_is_an_error(fast):
    graph = _unet(fast=fast)
    i = [b.name for b in graph].index("dec0.1")
    r0 = graph[i - 1].srcs[1]
    graph[i] = graph[i]._replace(srcs=graph[i].srcs + (r0,))
    with pytest.raises(RuntimeError, match="an upsampled tensor has one consumer in this graph"):
        E.route_gradients(graph, IMAGE, True)


def test_source_width_outside_the_fast_kernels_is_an_error():
    graph = _unet()
    graph[1] = graph[1]._replace(srcs=((1, 0, 48),))
    with pytest.raises(RuntimeError, match="enc0.1: mixed precision needs source widths of 32, 64 or 128 channels"):
        E.route_gradients(graph, IMAGE, True)


def test_pending_contribution_without_its_partner_is_an_error():
    """A PENDING contribution waits for a fast stride-2 conv that reads the same tensor.  The conditions that create it
    are the ones that reader tests, so the only graph that leaves it unsummed is one whose stride-2 reader is not
    walked between the decoder conv and the producer; it is refused before any kernel runs."""
    graph = [GraphBlock("down", Kind.FAST, 2, 64, 9, ((1, 0, 32),)),
             GraphBlock("stem", Kind.STEM, 3, 32, 1, ((IMAGE, 0, 1),)),
             GraphBlock("dec", Kind.FAST, 3, 32, 2, ((1, 0, 32),))]
    with pytest.raises(RuntimeError, match="a pending fp16 gradient was never summed"):
        E.route_gradients(graph, IMAGE, True)
