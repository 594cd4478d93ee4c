"""The registration contract of fa_mi355x/torch_op.py, on the CPU and without the
built library: the 46 schemas as literals, the overload order, the dispatch
keys, and for every overload its fake output, its CPU error and whether the
forward-only guard fires.  The literals are what the hand-written registrations
produced before the table replaced them."""
import pytest

torch = pytest.importorskip("torch")

from torch._subclasses.fake_tensor import FakeTensorMode  # noqa: E402

import torch_op_cases as C  # noqa: E402

SCHEMAS = [
    'fa_mi355x::attn_bshd(Tensor q, Tensor k, Tensor v, bool causal=False) -> Tensor',
    'fa_mi355x::attn_bshd.window(Tensor q, Tensor k, Tensor v, bool causal=False, int window=0) -> Tensor',
    'fa_mi355x::attn_bshd.sinks(Tensor q, Tensor k, Tensor v, bool causal=False, int window=0, Tensor? sinks=None) -> Tensor',
    'fa_mi355x::attn_bshd_bwd(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor out, Tensor lse, bool causal=False) -> (Tensor, Tensor, Tensor)',
    'fa_mi355x::attn_bshd_bwd.window(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor out, Tensor lse, bool causal=False, int window=0) -> (Tensor, Tensor, Tensor)',
    'fa_mi355x::attn_bshd_bwd.sinks(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor out, Tensor lse, bool causal=False, int window=0, Tensor? sinks=None) -> (Tensor, Tensor, Tensor, Tensor)',
    'fa_mi355x::attn_bshd_fwd(Tensor q, Tensor k, Tensor v, bool causal=False) -> (Tensor, Tensor)',
    'fa_mi355x::attn_bshd_fwd.window(Tensor q, Tensor k, Tensor v, bool causal=False, int window=0) -> (Tensor, Tensor)',
    'fa_mi355x::attn_bshd_fwd.sinks(Tensor q, Tensor k, Tensor v, bool causal=False, int window=0, Tensor? sinks=None) -> (Tensor, Tensor)',
    'fa_mi355x::attn_varlen(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor? cu_seqlens_k=None, bool causal=False) -> Tensor',
    'fa_mi355x::attn_varlen.window(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor? cu_seqlens_k=None, bool causal=False, int window=0) -> Tensor',
    'fa_mi355x::attn_varlen.sinks(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor? cu_seqlens_k=None, bool causal=False, int window=0, Tensor? sinks=None) -> Tensor',
    'fa_mi355x::attn_varlen_bwd(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor out, Tensor lse, Tensor cu_seqlens_q, Tensor? cu_seqlens_k=None, bool causal=False) -> (Tensor, Tensor, Tensor)',
    'fa_mi355x::attn_varlen_bwd.window(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor out, Tensor lse, Tensor cu_seqlens_q, Tensor? cu_seqlens_k=None, bool causal=False, int window=0) -> (Tensor, Tensor, Tensor)',
    'fa_mi355x::attn_varlen_bwd.sinks(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor out, Tensor lse, Tensor cu_seqlens_q, Tensor? cu_seqlens_k=None, bool causal=False, int window=0, Tensor? sinks=None) -> (Tensor, Tensor, Tensor, Tensor)',
    'fa_mi355x::attn_varlen_fwd(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor? cu_seqlens_k=None, bool causal=False) -> (Tensor, Tensor)',
    'fa_mi355x::attn_varlen_fwd.window(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor? cu_seqlens_k=None, bool causal=False, int window=0) -> (Tensor, Tensor)',
    'fa_mi355x::attn_varlen_fwd.sinks(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor? cu_seqlens_k=None, bool causal=False, int window=0, Tensor? sinks=None) -> (Tensor, Tensor)',
    'fa_mi355x::cache_append(Tensor k_new, Tensor v_new, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor kv_lens, Tensor? new_lens=None, Tensor? k_scale=None, Tensor? v_scale=None) -> ()',
    'fa_mi355x::cache_append_paged(Tensor k_new, Tensor v_new, Tensor(a!) k_pages, Tensor(b!) v_pages, Tensor block_table, Tensor kv_lens, Tensor? new_lens=None, Tensor? k_scale=None, Tensor? v_scale=None) -> ()',
    'fa_mi355x::cache_append_varlen(Tensor k_new, Tensor v_new, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor cu_seqlens, Tensor kv_lens, Tensor? k_scale=None, Tensor? v_scale=None) -> ()',
    'fa_mi355x::cache_append_varlen_paged(Tensor k_new, Tensor v_new, Tensor(a!) k_pages, Tensor(b!) v_pages, Tensor block_table, Tensor cu_seqlens, Tensor kv_lens, Tensor? k_scale=None, Tensor? v_scale=None) -> ()',
    'fa_mi355x::decode(Tensor q, Tensor k_cache, Tensor v_cache, Tensor? kv_lens=None, bool causal=True, Tensor? k_scale=None, Tensor? v_scale=None) -> Tensor',
    'fa_mi355x::decode.window(Tensor q, Tensor k_cache, Tensor v_cache, Tensor? kv_lens=None, bool causal=True, Tensor? k_scale=None, Tensor? v_scale=None, int window=0) -> Tensor',
    'fa_mi355x::decode.sinks(Tensor q, Tensor k_cache, Tensor v_cache, Tensor? kv_lens=None, bool causal=True, Tensor? k_scale=None, Tensor? v_scale=None, int window=0, Tensor? sinks=None) -> Tensor',
    'fa_mi355x::decode_paged(Tensor q, Tensor k_pages, Tensor v_pages, Tensor block_table, Tensor? kv_lens=None, bool causal=True) -> Tensor',
    'fa_mi355x::decode_paged.kv8(Tensor q, Tensor k_pages, Tensor v_pages, Tensor block_table, Tensor? kv_lens=None, bool causal=True, Tensor? k_scale=None, Tensor? v_scale=None) -> Tensor',
    'fa_mi355x::decode_paged.window(Tensor q, Tensor k_pages, Tensor v_pages, Tensor block_table, Tensor? kv_lens=None, bool causal=True, Tensor? k_scale=None, Tensor? v_scale=None, int window=0) -> Tensor',
    'fa_mi355x::decode_paged.sinks(Tensor q, Tensor k_pages, Tensor v_pages, Tensor block_table, Tensor? kv_lens=None, bool causal=True, Tensor? k_scale=None, Tensor? v_scale=None, int window=0, Tensor? sinks=None) -> Tensor',
    'fa_mi355x::fwd(Tensor q, Tensor k, Tensor v, bool causal=False) -> Tensor',
    'fa_mi355x::prefill(Tensor q, Tensor k_cache, Tensor v_cache, Tensor? kv_lens=None, Tensor? q_lens=None, bool causal=True, Tensor? k_scale=None, Tensor? v_scale=None) -> Tensor',
    'fa_mi355x::prefill.window(Tensor q, Tensor k_cache, Tensor v_cache, Tensor? kv_lens=None, Tensor? q_lens=None, bool causal=True, Tensor? k_scale=None, Tensor? v_scale=None, int window=0) -> Tensor',
    'fa_mi355x::prefill.sinks(Tensor q, Tensor k_cache, Tensor v_cache, Tensor? kv_lens=None, Tensor? q_lens=None, bool causal=True, Tensor? k_scale=None, Tensor? v_scale=None, int window=0, Tensor? sinks=None) -> Tensor',
    'fa_mi355x::prefill_paged(Tensor q, Tensor k_pages, Tensor v_pages, Tensor block_table, Tensor? kv_lens=None, Tensor? q_lens=None, bool causal=True, Tensor? k_scale=None, Tensor? v_scale=None) -> Tensor',
    'fa_mi355x::prefill_paged.window(Tensor q, Tensor k_pages, Tensor v_pages, Tensor block_table, Tensor? kv_lens=None, Tensor? q_lens=None, bool causal=True, Tensor? k_scale=None, Tensor? v_scale=None, int window=0) -> Tensor',
    'fa_mi355x::prefill_paged.sinks(Tensor q, Tensor k_pages, Tensor v_pages, Tensor block_table, Tensor? kv_lens=None, Tensor? q_lens=None, bool causal=True, Tensor? k_scale=None, Tensor? v_scale=None, int window=0, Tensor? sinks=None) -> Tensor',
    'fa_mi355x::prefill_varlen(Tensor q, Tensor k_cache, Tensor v_cache, Tensor cu_seqlens_q, Tensor? kv_lens=None, bool causal=True, Tensor? k_scale=None, Tensor? v_scale=None) -> Tensor',
    'fa_mi355x::prefill_varlen.window(Tensor q, Tensor k_cache, Tensor v_cache, Tensor cu_seqlens_q, Tensor? kv_lens=None, bool causal=True, Tensor? k_scale=None, Tensor? v_scale=None, int window=0) -> Tensor',
    'fa_mi355x::prefill_varlen.sinks(Tensor q, Tensor k_cache, Tensor v_cache, Tensor cu_seqlens_q, Tensor? kv_lens=None, bool causal=True, Tensor? k_scale=None, Tensor? v_scale=None, int window=0, Tensor? sinks=None) -> Tensor',
    'fa_mi355x::prefill_varlen_paged(Tensor q, Tensor k_pages, Tensor v_pages, Tensor block_table, Tensor cu_seqlens_q, Tensor? kv_lens=None, bool causal=True, Tensor? k_scale=None, Tensor? v_scale=None) -> Tensor',
    'fa_mi355x::prefill_varlen_paged.window(Tensor q, Tensor k_pages, Tensor v_pages, Tensor block_table, Tensor cu_seqlens_q, Tensor? kv_lens=None, bool causal=True, Tensor? k_scale=None, Tensor? v_scale=None, int window=0) -> Tensor',
    'fa_mi355x::prefill_varlen_paged.sinks(Tensor q, Tensor k_pages, Tensor v_pages, Tensor block_table, Tensor cu_seqlens_q, Tensor? kv_lens=None, bool causal=True, Tensor? k_scale=None, Tensor? v_scale=None, int window=0, Tensor? sinks=None) -> Tensor',
    'fa_mi355x::rope_append(Tensor q, Tensor k_new, Tensor v_new, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor kv_lens, Tensor cos, Tensor sin, Tensor? new_lens=None, bool interleaved=False, Tensor? k_scale=None, Tensor? v_scale=None) -> Tensor',
    'fa_mi355x::rope_append_paged(Tensor q, Tensor k_new, Tensor v_new, Tensor(a!) k_pages, Tensor(b!) v_pages, Tensor block_table, Tensor kv_lens, Tensor cos, Tensor sin, Tensor? new_lens=None, bool interleaved=False, Tensor? k_scale=None, Tensor? v_scale=None) -> Tensor',
    'fa_mi355x::rope_append_varlen(Tensor q, Tensor k_new, Tensor v_new, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor cu_seqlens, Tensor kv_lens, Tensor cos, Tensor sin, bool interleaved=False, Tensor? k_scale=None, Tensor? v_scale=None) -> Tensor',
    'fa_mi355x::rope_append_varlen_paged(Tensor q, Tensor k_new, Tensor v_new, Tensor(a!) k_pages, Tensor(b!) v_pages, Tensor block_table, Tensor cu_seqlens, Tensor kv_lens, Tensor cos, Tensor sin, bool interleaved=False, Tensor? k_scale=None, Tensor? v_scale=None) -> Tensor',
]

# fwd, decode*, prefill*, attn_varlen and attn_bshd: the Autograd fallthrough and the forward-only guard
FORWARD_ONLY = {"fwd", "decode", "decode_paged", "prefill", "prefill_paged", "prefill_varlen",
                "prefill_varlen_paged", "attn_varlen", "attn_bshd"}

# The fake outputs at torch_op_cases' shapes (padded q [1,2,4,64]): (shape, dtype, stride) of each tensor.
F16, F32 = torch.float16, torch.float32
_PAD = ((1, 2, 4, 64), F16, (512, 256, 64, 1))
_PACK = ((20, 2, 64), F16, (128, 64, 1))
_PACK_KV = ((20, 1, 64), F16, (64, 64, 1))
_BSHD = ((1, 20, 2, 64), F16, (2560, 128, 64, 1))
_BSHD_KV = ((1, 20, 1, 64), F16, (1280, 64, 64, 1))
_DSINKS = ((2,), F32, (1,))
FAKE_OUT = {"fwd": [_PAD], "decode": [_PAD], "decode_paged": [_PAD], "prefill": [_PAD], "prefill_paged": [_PAD],
            "prefill_varlen": [_PACK], "prefill_varlen_paged": [_PACK],
            "cache_append": [], "cache_append_paged": [], "cache_append_varlen": [], "cache_append_varlen_paged": [],
            "rope_append": [_PAD], "rope_append_paged": [_PAD], "rope_append_varlen": [_PACK],
            "rope_append_varlen_paged": [_PACK],
            "attn_varlen": [_PACK], "attn_varlen_fwd": [_PACK, ((2, 20), F32, (20, 1))],
            "attn_varlen_bwd": [_PACK, _PACK_KV, _PACK_KV],
            "attn_bshd": [_BSHD], "attn_bshd_fwd": [_BSHD, ((1, 2, 20), F32, (20, 20, 1))],  # the permuted view
            "attn_bshd_bwd": [_BSHD, _BSHD_KV, _BSHD_KV]}


@pytest.fixture(scope="module")
def ns():
    import fa_mi355x.torch_op  # noqa: F401

    return torch.ops.fa_mi355x


def _cases(new, ints):
    return C.cases(C.inputs(new, ints, 4, 4))


def _cpu_cases():
    return _cases(lambda s, d: torch.zeros(s, dtype=d), lambda v: torch.tensor(v, dtype=torch.int32))


def _tensors(r):
    return [] if r is None else [r] if isinstance(r, torch.Tensor) else list(r)


def test_the_46_schemas_are_the_registered_set(ns):
    packets = sorted({s.split("::")[1].split("(")[0].split(".")[0] for s in SCHEMAS})
    assert len(packets) == 21 and len(SCHEMAS) == 46
    registered = {n for n in torch._C._dispatch_get_all_op_names() if n.startswith("fa_mi355x::")}
    assert registered == {s.split("(")[0] for s in SCHEMAS}
    got =[str(getattr(getattr(ns, p), o)._schema) for p in packets for o in getattr(ns, p).overloads()]
    assert got == SCHEMAS
    assert {(p, o) for p, o, _ in _cpu_cases()} == {(p, o) for p in packets for o in getattr(ns, p).overloads()}


def test_overload_order(ns):
    assert ns.decode.overloads() == ["default", "window", "sinks"]
    assert ns.decode_paged.overloads() == ["default", "kv8", "window", "sinks"]
    assert ns.prefill.overloads() == ["default", "window", "sinks"]
    assert ns.attn_varlen_bwd.overloads() == ["default", "window", "sinks"]


def test_dispatch_keys(ns):
    has = torch._C._dispatch_has_kernel_for_dispatch_key
    autograd = 0
    for packet, overload, _ in _cpu_cases():
        full = "fa_mi355x::" + packet + ("" if overload == "default" else "." + overload)
        assert has(full, "CUDA") and has(full, "CPU") and has(full, "Meta"), full
        assert has(full, "Autograd") == (packet in FORWARD_ONLY), full
        autograd += has(full, "Autograd")
    assert autograd == 26


def test_every_overload_under_fake_tensor_mode(ns):
    with FakeTensorMode():
        rows = _cases(lambda s, d: torch.zeros(s, dtype=d, device="cuda"),
                      lambda v: torch.tensor(v, dtype=torch.int32, device="cuda"))
        for packet, overload, args in rows:
            out = _tensors(getattr(getattr(ns, packet), overload)(*args))
            want = FAKE_OUT[packet] + ([_DSINKS] if (packet[-4:], overload) == ("_bwd", "sinks") else [])
            assert [(tuple(t.shape), t.dtype, t.stride()) for t in out] == want, (packet, overload)
            assert all(t.device.type == "cuda" for t in out), (packet, overload)


def test_every_overload_refuses_cpu_tensors(ns):
    for packet, overload, args in _cpu_cases():
        with pytest.raises(ValueError) as e:
            getattr(getattr(ns, packet), overload)(*args)
        assert str(e.value) == "fa_mi355x::%s needs GPU tensors (no CPU path)" % packet, (packet, overload)


def test_autograd_functions_pick_the_overload_the_call_needs(ns, monkeypatch):
    """A plain call takes the default overload (not .window with W = 0), a window alone
    .window, sinks .sinks, in the forward and in the backward."""
    import types

    import fa_mi355x.torch_op as top

    calls = []

    def packet(name, result):
        def overload(which):
            def op(*args):
                calls.append((name, which, len(args)))
                return result(which)
            return op
        return types.SimpleNamespace(default=overload("default"), window=overload("window"), sinks=overload("sinks"))

    q = torch.zeros((20, 2, 64), dtype=F16)
    cu = torch.tensor([0, 20], dtype=torch.int32)
    sinks = torch.zeros(2, requires_grad=True)
    for layout, func, mid in (("varlen", top.flash_attn_varlen_func, (cu,)), ("bshd", top.flash_attn_func, ())):
        x = q if mid else q.view(1, 20, 2, 64)
        monkeypatch.setattr(top, "attn_%s_fwd" % layout, packet("fwd", lambda which: (x * 1, torch.zeros(2, 20))))
        monkeypatch.setattr(top, "attn_%s_bwd" % layout, packet("bwd", lambda which: (
            (x, x, x, torch.ones(2)) if which == "sinks" else (x, x, x))))
        n = 3 + (2 if mid else 0) + 1  # q, k, v, the cu_seqlens pair, causal
        for kw, which, more in (({}, "default", 0), ({"window": 3}, "window", 1), ({"sinks": sinks}, "sinks", 2),
                                ({"window": 3, "sinks": sinks}, "sinks", 2)):
            del calls[:]
            sinks.grad = None
            a, b, c = (x.clone().requires_grad_() for _ in range(3))
            func(a, b, c, *mid, causal=True, **kw).sum().backward()
            assert calls == [("fwd", which, n + more), ("bwd", which, n + 3 + more)], (layout, kw)
            assert a.grad is not None and (sinks.grad is not None) == ("sinks" in kw)


def test_forward_only_guard_on_exactly_the_guarded_ops(ns):
    rows = _cases(lambda s, d: torch.zeros(s, dtype=d, device="meta", requires_grad=d == F16),
                  lambda v: torch.zeros(torch.tensor(v).shape, dtype=torch.int32, device="meta"))
    message = ("fa_mi355x::fwd is forward-only (no backward): call it under torch.no_grad() / inference_mode "
               "or on tensors that do not require grad")
    for packet, overload, args in rows:
        op = getattr(getattr(ns, packet), overload)
        if packet in FORWARD_ONLY:
            with pytest.raises(RuntimeError) as e:
                op(*args)
            assert str(e.value) == message, (packet, overload)
            with torch.no_grad():
                out = _tensors(op(*args))
        else:
            out = _tensors(op(*args))
        assert [tuple(t.shape) for t in out][:len(FAKE_OUT[packet])] == [w[0] for w in FAKE_OUT[packet]]
