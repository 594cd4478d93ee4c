"""The reference's C++ host entry, driven on the GPU.

* The reference-style harness executable (tests/harness/, a rebuild of the
  reference's main(), flash_attention.cu:702-884: register report + the four
  correctness checks against the CPU oracle) runs with FA_SKIP_BENCH=1 and
  must print PASS on every check.
* The C++ symbol flash_attention_v9_dispatch (include/flash_attention_v9.h,
  the reference's signature :606-611) is called through its mangled name with
  NON-NULL split-K buffers: like the reference it must ignore them (they keep
  their sentinel bytes) and produce the oracle's output.
"""
import ctypes
import os
import subprocess

import pytest

torch = pytest.importorskip("torch")

import oracle  # noqa: E402  (test infrastructure)
from fwd_helpers import rand_half as _rand, to_dev as _dev, to_host_bits as _bits  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "harness", "build", "flash_attention")
V9_MANGLED = "_Z27flash_attention_v9_dispatchPK6__halfS1_S1_PS_PfS3_iiiibP12ihipStream_t"


def test_reference_harness_checks_pass():
    assert os.path.exists(HARNESS), f"{HARNESS} not built (__graft_entry__.build())"
    env = dict(os.environ, FA_SKIP_BENCH="1", FA_COOLDOWN_S="0")
    r = subprocess.run([HARNESS], env=env, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    checks = [ln for ln in out.splitlines() if "max_diff=" in ln]
    assert len(checks) >= 4, out[-4000:]  # the reference's four checks (:757-884), at least
    assert all(ln.count("PASS") == 2 for ln in checks), "\n".join(checks)


@pytest.mark.parametrize("causal", [False, True])
def test_v9_dispatch_ignores_splitk_buffers(causal):
    import fa_mi355x

    lib = fa_mi355x.load_library()
    fn = getattr(lib, V9_MANGLED)
    vp, i = ctypes.c_void_p, ctypes.c_int
    fn.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, i, ctypes.c_bool, vp]
    fn.restype = None
    b, h, s, d = 1, 8, 300, 128
    q, k, v = oracle.gen_inputs(b, h, s, d, 42)
    ref = oracle.attention(q, k, v, causal)
    dq, dk, dv = _dev(q), _dev(k), _dev(v)
    o = torch.empty_like(dq)
    # deliberately tiny split-K buffers: any write into them would be out of bounds
    sentinel = float.fromhex("0x1.5555p-3")
    buf_o = torch.full((64,), sentinel, dtype=torch.float32, device="cuda")
    buf_ml = torch.full((64,), sentinel, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    fn(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), o.data_ptr(), buf_o.data_ptr(),
       buf_ml.data_ptr(), b, h, s, d, causal, stream)
    torch.cuda.synchronize()
    assert oracle.max_abs_diff(_bits(o), ref) <= 1e-3
    assert bool((buf_o == sentinel).all()) and bool((buf_ml == sentinel).all())


def _v9(lib):
    fn = getattr(lib, V9_MANGLED)
    vp, i = ctypes.c_void_p, ctypes.c_int
    fn.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, i, ctypes.c_bool, vp]
    fn.restype = None
    return fn


# (B, H, S, causal, what the dispatcher runs): the shapes whose tier needs a
# workspace, and two that need none
V9_TIER_SHAPES = [
    (1, 4, 8192, True, "split"),
    (1, 2, 16384, True, "split"),
    (32, 32, 4096, True, "pool"),
    (1, 32, 1024, True, "plain"),
    (2, 3, 1000, False, "plain"),
]


@pytest.mark.parametrize("b,h,s,causal,kind", V9_TIER_SHAPES)
def test_v9_dispatch_runs_the_workspace_tiers(b, h, s, causal, kind):
    """verdict r05 item 6: the reference signature runs the same tier as the
    workspace entries (the causal split tier, the W4 tail pool) through the
    wrapper's own (device, stream) workspace -- bit-identical outputs"""
    import fa_mi355x

    lib = fa_mi355x.load_library()
    pieces = lib.fa_fwd_split_pieces(b, h, s, 128, int(causal))
    need = lib.fa_fwd_ws_bytes(b, h, s, 128, int(causal), 0)
    assert (pieces > 0) == (kind == "split") and (need == 65536) == (kind == "pool")
    q, k, v = (_rand((b, h, s, 128), 300 + i) for i in range(3))
    ref = fa_mi355x.flash_attention_fwd(q, k, v, causal)
    o = torch.empty_like(q)
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(2):  # the workspace is reused: its counters come back to zero
        o.zero_()
        _v9(lib)(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), None, None, b, h, s, 128, causal, st)
        torch.cuda.synchronize()
        assert torch.equal(o, ref)


def test_v9_dispatch_under_graph_capture():
    """captured on a stream the wrapper has no workspace for: it allocates
    nothing during capture and runs the workspace-free tier (here the KV-quad
    instead of the split tier); replays match an eager call of that tier"""
    import fa_mi355x

    lib = fa_mi355x.load_library()
    b, h, s = 1, 4, 8192
    q, k, v = (_rand((b, h, s, 128), 400 + i) for i in range(3))
    o = torch.empty_like(q)
    ref = torch.empty_like(q)
    side = torch.cuda.Stream()
    eager = torch.cuda.Stream()
    with torch.cuda.stream(eager):
        assert lib.fa_fwd_f16(q.data_ptr(), k.data_ptr(), v.data_ptr(), ref.data_ptr(), b, h, s, 128, 1,
                              eager.cuda_stream) == 0
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        _v9(lib)(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), None, None, b, h, s, 128, True,
                 side.cuda_stream)
    for _ in range(2):
        o.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(o, ref)
