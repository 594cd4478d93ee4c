"""Every overload of torch.ops.fa_mi355x.* against the fa_mi355x function it
wraps, bit for bit, at the smallest shapes (torch_op_cases.py); the contiguity
rule (a strided argument that is not as-is is copied, a strided cache raises);
and the two autograd functions against the explicit _fwd / _bwd overloads.
Every input is valid or refused on the host before a launch."""
import pytest

torch = pytest.importorskip("torch")

import torch_op_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

_IDS = [p + "." + o for p, o, _ in C.cases(C.inputs(lambda s, d: torch.zeros(s, dtype=d),
                                                    lambda v: torch.tensor(v, dtype=torch.int32), 1, 5))]


@pytest.fixture(scope="module")
def fa():
    import fa_mi355x
    import fa_mi355x.torch_op  # noqa: F401

    return fa_mi355x


@pytest.fixture(scope="module")
def rows(fa):
    g = torch.Generator().manual_seed(7)
    t = C.inputs(lambda s, d: torch.randn(s, generator=g).to(d).cuda(),
                 lambda v: torch.tensor(v, dtype=torch.int32, device="cuda"), 1, 5)
    return {p + "." + o: (p, o, args) for p, o, args in C.cases(t)}


def _clone(x):
    return x.clone() if isinstance(x, torch.Tensor) else x


def _tensors(r):
    return [] if r is None else [r] if isinstance(r, torch.Tensor) else list(r)


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x.view(torch.uint8) if x.dtype is C.F8 else x,
                                                y.view(torch.uint8) if y.dtype is C.F8 else y)
                                    for x, y in zip(a, b))


def _strided(x):
    """x's values in a view that is not contiguous."""
    y = torch.stack([x, x], -1)[..., 0]
    assert not y.is_contiguous() and torch.equal(x, y)
    return y


def _call(fa, packet, overload, args):
    """The op on clones of args -> (what it returned, its tensor arguments after the call)."""
    args = [_clone(a) for a in args]
    got = getattr(getattr(torch.ops.fa_mi355x, packet), overload)(*args)
    return _tensors(got), [a for a in args if isinstance(a, torch.Tensor)]


def _keywords(fa, packet, overload, args):
    """args by the schema's names; a backward gets the out and lse of its own forward."""
    schema = getattr(getattr(torch.ops.fa_mi355x, packet), overload)._schema
    kw = dict(zip([a.name for a in schema.arguments], args))
    if packet.endswith("_bwd"):
        fwd = getattr(fa, C.WRAPPED[packet[:-4]][0])
        kw["out"], kw["lse"] = fwd(**{n: x for n, x in kw.items() if n not in ("dout", "out", "lse")},
                                   return_lse=True)
    return kw


@pytest.mark.parametrize("case", _IDS)
def test_overload_is_the_wrapped_function(fa, rows, case):
    packet, overload, args = rows[case]
    kw = _keywords(fa, packet, overload, args)
    got, after = _call(fa, packet, overload, list(kw.values()))
    name, extra = C.WRAPPED[packet]
    mine = {n: _clone(x) for n, x in kw.items()}
    want = _tensors(getattr(fa, name)(**mine, **extra))
    torch.cuda.synchronize()
    assert _same(got, want)
    assert _same(after, [x for x in mine.values() if isinstance(x, torch.Tensor)])  # the caches too


@pytest.mark.parametrize("case,arg", [("decode.default", 0), ("prefill.window", 0), ("cache_append.default", 0),
                                      ("rope_append_paged.default", 0), ("attn_varlen.sinks", 3),
                                      ("attn_varlen_bwd.default", 6)])
def test_a_strided_argument_that_is_not_as_is_is_copied(fa, rows, case, arg):
    packet, overload, args = rows[case]
    args = list(_keywords(fa, packet, overload, args).values())
    want = _call(fa, packet, overload, args)
    args[arg] = _strided(args[arg])
    got = _call(fa, packet, overload, args)
    torch.cuda.synchronize()
    assert _same(got[0], want[0]) and _same(got[1], want[1])


@pytest.mark.parametrize("case", ["decode.default", "decode.sinks", "prefill_varlen.window", "cache_append.default",
                                  "rope_append.default"])
def test_a_strided_cache_still_raises(fa, rows, case):
    packet, overload, args = rows[case]
    at = [i for i, a in enumerate(args) if a is rows["decode.default"][2][1]][0]  # k_cache
    wide = torch.zeros((1, C.HKV, C.CAP, 2 * C.D), dtype=C.F16, device="cuda")
    args = list(args)
    args[at] = wide[..., :C.D]  # a slice of a larger cache
    assert not args[at].is_contiguous()
    with pytest.raises(fa.FlashAttentionError):
        getattr(getattr(torch.ops.fa_mi355x, packet), overload)(*args)
    assert not wide.any()  # nothing was written


@pytest.mark.parametrize("layout", ["varlen", "bshd"])
@pytest.mark.parametrize("window,with_sinks", [(0, False), (3, False), (0, True), (3, True)])
def test_autograd_function_is_the_explicit_overloads(fa, rows, layout, window, with_sinks):
    ops = torch.ops.fa_mi355x
    fwd_args = rows["attn_%s_fwd.default" % layout][2]
    (q, k, v), mid = (x.clone().requires_grad_() for x in fwd_args[:3]), fwd_args[3:-1]
    dout = rows["attn_%s_bwd.default" % layout][2][0]
    sinks = rows["attn_varlen.sinks"][2][-1].clone().requires_grad_() if with_sinks else None
    func = fa.flash_attn_varlen_func if layout == "varlen" else fa.flash_attn_func
    out = func(q, k, v, *mid, causal=True, window=window, sinks=sinks)
    out.backward(dout)

    fwd, bwd = getattr(ops, "attn_%s_fwd" % layout), getattr(ops, "attn_%s_bwd" % layout)
    overload, tail = (("sinks", (window, sinks)) if with_sinks else ("window", (window,)) if window
                      else ("default", ()))
    with torch.no_grad():
        o, lse = getattr(fwd, overload)(q, k, v, *mid, True, *tail)
        grads = getattr(bwd, overload)(dout, q, k, v, o, lse, *mid, True, *tail)
    torch.cuda.synchronize()
    assert _same([out.detach(), q.grad, k.grad, v.grad], [o, *grads[:3]])
    if with_sinks:
        assert len(grads) == 4 and torch.equal(sinks.grad, grads[3])
    else:
        assert len(grads) == 3
