"""Every gemm16 instantiation at its dispatch and pipeline edges (GPU), against the fp64 plane references of tests/op_refs.py.

The dispatch tables of csrc/gemm16_small_*.hip / gemm16_t3_*.hip are restated below (TILE_DIMS, RING -> INST) and the case tables are
built from them; _check_tables() fails at import if an instantiation has no case.  Launches that ops.gemm16 cannot express (strided,
canaried, misaligned, batched) are built with GemmArgs + ops.gemm16_raw by the local helper _launch().

Entry point / path -> test
  launch<T, 128, 128, 32, 2, 2, AP, WP, NS>   (tile 1; passes 1 / 2 / 3 / 6 = NS 4 / 3 / 2 / 3; f16 and bf16)
  launch<T, 128,  64, 32, 2, 2, AP, WP, NS>   (tile 2; NS 4 / 3 / 3 / 3)
  launch<T, 256, 256, 32, 2, 4, AP, WP, NS>   (tile 3; NS 4 / 3 / 2 / 3)
      all 24: test_instantiation_k_pipeline[dtype-tile-passes]: the LDS-DMA loader <GLDS, NS> at nk = 1 .. 5 slabs, the
      register-staged loader <false, 2> at K = 8 / 24 / 40 / 72 and under gemm_glds = 0, the <GLDS, 2> A/B kernel under gemm_glds = 2,
      the corner shapes; operands are views of NaN-padded buffers
  launch<f16, 256, 256, 32, 4, 2, 1, 1, MX_NS, true> (passes 4)    test_mx_kernel_group_parities
  epilogue() vector / scalar branch, epilogue_pk(), epilogue32()   test_epilogue_matrix[tile-dtype-path] (strided + canaried outputs,
      every output set x bias kind x activation x residual kind; specialised == generic bit for bit)
  head-major scatter (hm_T)               test_headmajor_output, test_headmajor_needs_the_vector_epilogue
  nbatch / nb_inner / *_so / *_si         test_batched_launch[tile-dtype-passes-path]
  a_rows_per_batch / a_batch_stride       test_implicit_conv_rows
  tile == 0 rule of mer_gemm16            test_auto_tile_rule (R.auto_tile is pinned on the CPU in test_op_refs_cpu.py)
  dispatch_p<T> at TM = 4 and TM = 3 (gemm16p_kernel<T, EPI 0 / 1 / 2, ACT, TM>)   test_persistent_smallest[dtype-tm-N-K]

References.  R.gemm16_planes_ref sums, in fp64, exactly the plane products the kernel accumulates, on the rounded planes: no input
rounding is left for the tolerance to carry, so the project's 2e-5 max-norm bound on an fp32 output (test_gemm16_single_pass /
test_gemm16_three_pass_is_fp32_grade in tests/test_ops_gpu.py) serves every dtype and pass count.  Input family "indep"
(R.indep_planes): the lo planes are independent random planes, every product term is of order 1, and a dropped or mis-paired pass
moves the result by tens of percent (asserted on the CPU, test_indep_planes_discriminate_every_pass_set).  quick_gelu / gelu_tanh:
max(2e-5, 2 x model), model = the error of a torch-fp32 restatement of csrc/common.h on the same pre-activations (R.act_bound), printed
in every failure.  16-bit outputs are bounded elementwise from round-to-nearest (u = 2^-11 / 2^-8; pairs 2^-21 / 2^-16):
|hi - ref| <= u |ref| + 2e-5 max|ref| + 2^-25, and where c32 is also requested hi == round16(c32), lo == round16(c32 - hi) exactly.

What test_auto_tile_rule can and cannot see: every tile class feeds an accumulator the same MFMA sequence, so the three forced
launches agree bit for bit with each other as well; the test pins that the kernel the rule picks is correct at the rule's edges (the
narrowest 128x128 launch, the shortest 256x256 one, passes 4 without an MX plane on either side of N = 192), not which one it picked.
"""
import ctypes
import functools
import json
import types

import pytest
import torch

import op_refs as R
from util import bf8_round, mx_decode

pytestmark = pytest.mark.gpu

DTYPES = ("f16", "bf16")
PASSES = (1, 2, 3, 6)
TILE_DIMS = {1: (128, 128), 2: (128, 64), 3: (256, 256)}          # mer_gemm16_args.tile -> (BM, BN)
# (tile, passes) -> NS, the last template argument of the launch<> lines (the same in the f16 and the bf16 files)
RING = {(1, 1): 4, (1, 2): 3, (1, 3): 2, (1, 6): 3,
        (2, 1): 4, (2, 2): 3, (2, 3): 3, (2, 6): 3,
        (3, 1): 4, (3, 2): 3, (3, 3): 2, (3, 6): 3}
INST = {(d, t, p): TILE_DIMS[t] + (RING[t, p],) for d in DTYPES for t in TILE_DIMS for p in PASSES}
MX_INST = ("f16", 3, 4)                                           # launch<f16, 256, 256, 32, 4, 2, 1, 1, MX_NS = 3, true>
GLDS_NK = (1, 2, 3, 4, 5)                                         # K = 32 nk through the LDS-DMA ring
REG_K = (8, 24, 40, 72)                                           # K % 32 != 0: the register-staged loader (1, 1, 2 and 3 slabs)
AB_K = (96, 160)                                                  # gemm_glds = 0 / 2 against the default loader
ACTS = (None, "gelu", "quick_gelu", "gelu_tanh", "relu")
OUTSETS = (("c32",), ("c16",), ("c16", "lo"), ("c32", "c16"), ("c32", "c16", "lo"))
BIASES = ("none", "static", 1, 7, 50)                             # an int: a table with that many rows per sequence
PATHS = ("vec", "scalar_n", "scalar_ld32", "scalar_ptr16")
MER_ESHAPE = -2


def _corners(BM, BN):
    return ((1, 8, 8), (BM, BN, 32), (BM + 1, BN + 3, 40), (2 * BM + 1, 1, 32))


def _check_tables():
    assert len(INST) == 24 and set(RING) == {(t, p) for t in TILE_DIMS for p in PASSES}
    for (dtype, tile, passes), (BM, BN, NS) in INST.items():
        D = NS - 1                                                # prefetch distance: the prologue / vmcnt branches are nk >= D, kt + D < nk
        assert D in (1, 2, 3)
        assert {D, D + 1} <= set(GLDS_NK) and (D == 1 or any(nk < D for nk in GLDS_NK)), (tile, passes)
        assert any(nk > NS for nk in GLDS_NK), "no K wraps the ring"
        assert all(32 * nk % 32 == 0 for nk in GLDS_NK) and all(k % 8 == 0 and k % 32 for k in REG_K)
        assert {(k + 31) // 32 % 2 for k in REG_K} == {0, 1} and min(REG_K) < 32 < max(REG_K)       # both buffer parities
        assert all(k % 32 == 0 and k // 32 in GLDS_NK for k in AB_K)                                # ... have a default launch to equal
    assert set(_instantiation_ids()) == {f"{d}-t{t}-p{p}" for d, t, p in INST}, "an instantiation has no case"


def _instantiation_ids():
    return [f"{d}-t{t}-p{p}" for d, t, p in sorted(INST)]


_check_tables()


def _ops():
    from mertools_amd import ops
    return ops


def _lib():
    from mertools_amd import _lib as L
    return L.lib()


class _option:
    """mer_set_option for the body of a with-block; the previous value is put back on the way out."""

    def __init__(self, name, value):
        self.name, self.value = name.encode(), value

    def __enter__(self):
        old = ctypes.c_int(0)
        assert _lib().mer_get_option(self.name, ctypes.byref(old)) == 0
        self.old = old.value
        assert _lib().mer_set_option(self.name, self.value) == 0

    def __exit__(self, *exc):
        _lib().mer_set_option(self.name, self.old)


def _profiled(fn):
    """Runs fn() under the library's launch profiler -> {kernel label: launches} (gemm16, gemm16_w2, gemm16_x3, gemm16_mx, gemm16p)."""
    lib = _lib()
    buf = ctypes.create_string_buffer(1 << 14)
    lib.mer_prof_enable(1)
    try:
        fn()
    finally:
        lib.mer_prof_report(buf, len(buf))
        lib.mer_prof_enable(0)
    return {r["name"]: r["calls"] for r in json.loads(buf.value.decode())}


# ------------------------------------------------------------------------------------------------------ operands and windows
def _padded(t, extra, dev):
    """The device copy of a 16-bit [rows, K] plane as a view of a [rows + 2, K + extra] buffer of NaN: a loader that reads past K or
    past the last row turns the output non-finite."""
    rows, K = t.shape
    buf = torch.full((rows + 2, K + extra), float("nan"), dtype=t.dtype)
    buf[:rows, :K] = t
    return buf.to(dev)[:rows, :K]


@functools.lru_cache(maxsize=64)
def _cpu_planes(M, N, K, dtype, seed=0):
    return R.indep_planes(M, N, K, dtype, 7000 + seed + 3 * M + 5 * N + 7 * K)


class _Planes:
    def __init__(self, dev, M, N, K, dtype, seed=0):
        self.cpu = _cpu_planes(M, N, K, dtype, seed)
        self.a_hi, self.a_lo = _padded(self.cpu[0], 8, dev), _padded(self.cpu[1], 8, dev)          # lda = K + 8
        self.w_hi, self.w_lo = _padded(self.cpu[2], 16, dev), _padded(self.cpu[3], 16, dev)        # ldw = K + 16

    def ref(self, passes, M=None):
        ah, al, wh, wl = self.cpu
        return R.gemm16_planes_ref(ah[:M], al[:M], wh, wl, passes)


class _Win:
    """An [M, N] window with row stride ld inside a flat canary-filled buffer, eight rows of canary in front and behind; `off` moves
    its first element that many elements off 16-byte alignment.  kind: "f32" or a 16-bit dtype name."""

    def __init__(self, dev, kind, M, N, ld, off=0, data=None):
        assert ld >= N
        self.kind, self.shape, self.ld = kind, (M, N), ld
        self.start = 8 * ld + off
        n = self.start + (M - 1) * ld + N + 8 * ld
        self.flat = torch.full((n,), R.CANARY32, device=dev) if kind == "f32" else R.canary16((n,), kind, dev)
        self.view = torch.as_strided(self.flat, (M, N), (ld, 1), self.start)
        assert (self.view.data_ptr() % 16 == 0) == (off % (4 if kind == "f32" else 8) == 0)
        if data is not None:
            self.view.copy_(data.to(dev))

    def ptr(self):
        return self.view.data_ptr()

    def untouched_outside(self):
        c = self.flat.clone()
        if self.kind == "f32":
            torch.as_strided(c, self.shape, (self.ld, 1), self.start).fill_(R.CANARY32)
            return R.is_canary32(c)
        c = c.view(torch.int16)
        torch.as_strided(c, self.shape, (self.ld, 1), self.start).fill_(0x7B7B)
        return bool((c == 0x7B7B).all())

    def untouched(self):
        return R.is_canary32(self.flat) if self.kind == "f32" else R.is_canary16(self.flat)


def _args(P, M, N, K, dtype, passes, tile, *, c32=None, c16=None, lo=None, bias=None, table=None, seg=0, act=None, residual=None,
          headmajor=None, **fields):
    """GemmArgs of one launch: P holds the operand planes (any 2-D views), c32 / c16 / lo / residual / table are _Win objects."""
    ops = _ops()
    g = ops.GemmArgs()
    g.M, g.N, g.K, g.dtype = M, N, K, ops.dt_code(dtype)
    g.a_hi, g.lda = P.a_hi.data_ptr(), P.a_hi.stride(0)
    g.w_hi, g.ldw = P.w_hi.data_ptr(), P.w_hi.stride(0)
    if passes in (3, 6):
        g.a_lo = P.a_lo.data_ptr()
    if passes in (2, 3, 4):
        g.w_lo = P.w_lo.data_ptr()
    if table is not None:
        g.bias, g.bias_seg_rows, g.bias_ld = table.ptr(), seg, table.ld
    elif bias is not None:
        g.bias = bias.data_ptr()
    g.act = ops.ACT[act]
    if residual is not None:
        g.residual, g.ldr = residual.ptr(), residual.ld
    if c32 is not None:
        g.c32, g.ldc32 = c32.ptr(), c32.ld
    if c16 is not None:
        g.c16_hi, g.ldc16 = c16.ptr(), c16.ld
    if lo is not None:
        assert lo.ld == c16.ld
        g.c16_lo = lo.ptr()
    g.nbatch, g.nb_inner, g.passes, g.tile = 1, 1, passes, tile
    if headmajor is not None:
        g.headmajor_T, g.headmajor_H = headmajor
    for k, v in fields.items():
        setattr(g, k, v)
    return g


def _launch(*a, **kw):
    _ops().gemm16_raw(_args(*a, **kw))


def _err32(out, ref):
    """max|out - ref| / max|ref| with both on the device (ref: fp64)."""
    return ((out.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def _assert32(win, ref_d, bound, what, model=0.0):
    out = win.view
    assert bool(torch.isfinite(out).all()), f"{what}: non-finite fp32 output"
    e = _err32(out, ref_d)
    assert e <= bound, f"{what}: c32 max-norm rel err {e:.3e} > bound {bound:.2e} (fp32 model of the activation: {model:.3e})"
    assert win.untouched_outside(), f"{what}: c32 written outside its [M, N] window"
    return e


def _assert16(hi, lo, ref_d, dtype, what, layout=None):
    """Elementwise round-to-nearest bounds of a 16-bit plane (and of the hi + lo pair); layout maps the row-major reference to the
    layout of the planes (head-major)."""
    ref = ref_d if layout is None else layout(ref_d)
    m = ref.abs().max().item()
    floor = R.GEMM_TOL * m + 2.0 ** -25
    h = hi.double()
    assert bool(torch.isfinite(h).all()), f"{what}: non-finite 16-bit output"
    over = ((h - ref).abs() - (R.U16[dtype] * ref.abs() + floor)).max().item()
    assert over <= 0.0, f"{what}: c16_hi is {over:.3e} past u |ref| + 2e-5 max|ref| + 2^-25 (max|ref| {m:.3e})"
    if lo is not None:
        over = ((h + lo.double() - ref).abs() - (R.U_PAIR[dtype] * ref.abs() + floor)).max().item()
        assert over <= 0.0, f"{what}: c16 hi + lo is {over:.3e} past u_pair |ref| + 2e-5 max|ref| + 2^-25 (max|ref| {m:.3e})"


def _assert_planes_of(c32, hi, lo, dtype, what):
    """The tolerance-free invariant of a launch that writes fp32 and 16-bit outputs: the planes are the split of the fp32 value."""
    want_hi = R.round16(c32, dtype)
    assert torch.equal(hi.view(torch.int16), want_hi.view(torch.int16)), f"{what}: c16_hi != round16(c32)"
    if lo is not None:
        want_lo = R.round16(c32 - want_hi.float(), dtype)
        assert torch.equal(lo.view(torch.int16), want_lo.view(torch.int16)), f"{what}: c16_lo != round16(c32 - c16_hi)"


# ------------------------------------------------------------------------------- B. instantiation x K-pipeline matrix
def _ld32(N):
    return (N + 3) // 4 * 4 + 4


@pytest.mark.parametrize("dtype,tile,passes", sorted(INST), ids=_instantiation_ids())
def test_instantiation_k_pipeline(dev, dtype, tile, passes):
    BM, BN, NS = INST[dtype, tile, passes]
    M0, N0 = BM + 1, BN + 8                                       # two tiles each way, ragged, vector epilogue
    shapes = [(M0, N0, 32 * nk, f"dma nk={nk} (D={NS - 1})") for nk in GLDS_NK]
    shapes += [(M0, N0, K, f"reg K={K}") for K in REG_K]
    shapes += [(M, N, K, "corner") for M, N, K in _corners(BM, BN)]
    runs = []
    for M, N, K, tag in shapes:
        P = _Planes(dev, M, N, K, dtype)
        wins = [_Win(dev, "f32", M, N, _ld32(N)) for _ in range(2)]
        for w in wins:
            _launch(P, M, N, K, dtype, passes, tile, c32=w)
        runs.append((M, N, K, tag, P, wins, None))
        if K in AB_K and (M, N) == (M0, N0):
            for glds in (0, 2) if NS > 2 else (0,):              # (NS == 2: gemm_glds = 2 is the default kernel itself)
                ab = [_Win(dev, "f32", M, N, _ld32(N)) for _ in range(2)]
                with _option("gemm_glds", glds):
                    for w in ab:
                        _launch(P, M, N, K, dtype, passes, tile, c32=w)
                runs.append((M, N, K, f"gemm_glds={glds}", P, ab, wins[0]))
    torch.cuda.synchronize()
    for M, N, K, tag, P, wins, default in runs:
        what = f"gemm16 {dtype} tile {tile} passes {passes} ({M}, {N}, {K}) {tag}"
        ref = P.ref(passes).to(dev)
        e = _assert32(wins[0], ref, R.GEMM_TOL, what)
        print(f"{what}: err {e:.3e}")
        if len(wins) == 2:
            assert wins[1].untouched_outside(), what
            assert torch.equal(wins[0].view, wins[1].view), f"{what}: two launches of the same case differ"
        if default is not None:
            assert torch.equal(wins[0].view, default.view), f"{what}: differs from the default loader (same MFMA sequence per accumulator)"


@pytest.mark.parametrize("K", [128, 256, 384])
def test_mx_kernel_group_parities(dev, K):
    """passes 4 on one, two and three 128-k groups (both group-buffer parities), against the fp64 emulation built from the packed plane
    by the independent decoder of tests/util.py, at the project's 3e-6 (test_gemm16_mx_corrected)."""
    ops = _ops()
    dtype, tile, passes = MX_INST
    for N in (200, 264):
        w = R.rand((N, K), 8100 + N + K, 0.05)
        wh, wl = R.split_planes(w, "f16")
        packed = ops.mx_pack(w - wh.float())
        wdec = mx_decode(packed, N, K)
        for M in (1, 65, 257):
            a = R.rand((M, K), 8200 + M).half()
            P = types.SimpleNamespace()
            P.a_hi, P.w_hi, P.w_lo = _padded(a, 8, dev), _padded(wh, 16, dev), _padded(wl, 16, dev)
            wins = [_Win(dev, "f32", M, N, _ld32(N)) for _ in range(2)]
            mx = packed.to(dev)

            def run():
                for w_ in wins:
                    _launch(P, M, N, K, dtype, passes, tile, c32=w_, w_mx=mx.data_ptr())
            assert _profiled(run) == {"gemm16_mx": 2}, "the launch did not take the MX kernel"
            emu = (a.double() @ wh.double().T + bf8_round(a) @ wdec.T).to(dev)
            what = f"gemm16 mx ({M}, {N}, {K})"
            e = _assert32(wins[0], emu, 3e-6, what)
            print(f"{what}: err {e:.3e}")
            assert wins[1].untouched_outside() and torch.equal(wins[0].view, wins[1].view), f"{what}: two launches differ"


# ---------------------------------------------------------------------------------- C. epilogue matrix, strided + canaried
def _path_geometry(path, BN):
    """-> N, ldc32, ldc16, ldr, element offset of c16_hi."""
    if path == "vec":
        N = BN + 8
        return N, N + 8, N + 8, N + 8, 0
    if path == "scalar_n":                                        # N % 8 != 0
        N = BN + 3
        return N, N + 5, N + 5, N + 5, 0
    N = BN + 8
    if path == "scalar_ld32":                                     # ldc32 (and ldr) % 4 != 0
        return N, N + 1, N + 8, N + 1, 0
    return N, N + 8, N + 8, N + 8, 1                              # scalar_ptr16: c16_hi one element off 16-byte alignment


def _residual_kinds(outs):
    return ("absent", "separate", "inplace") if "c32" in outs else ("absent", "separate")


def _defeats_vec(path, outs, res):
    """Whether this launch really takes the path the case is named after (the others would repeat a vector case)."""
    if path == "scalar_ld32":
        return "c32" in outs or res != "absent"
    if path == "scalar_ptr16":
        return "c16" in outs
    return True


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile", sorted(TILE_DIMS))
def test_epilogue_matrix(dev, tile, dtype, path):
    BM, BN = TILE_DIMS[tile]
    M, K, passes = BM + 1, 64, 1
    N, ld32, ld16, ldr, off16 = _path_geometry(path, BN)
    P = _Planes(dev, M, N, K, dtype, seed=1)
    z = P.ref(passes)
    bias = R.rand((N,), 9001)
    res = R.rand((M, N), 9002)
    bias_d, res_d = bias.to(dev), res.to(dev)
    ldt = (N + 3) // 4 * 4 + 4
    tables = {seg: R.rand(((M + seg - 1) // seg, N), 9100 + seg) for seg in BIASES if isinstance(seg, int)}
    n_launch = 0
    for bk in BIASES:
        kwb, tab = {}, None
        if bk == "static":
            kwb = dict(bias=bias_d)
        elif bk != "none":
            tab = _Win(dev, "f32", tables[bk].shape[0], N, ldt, data=tables[bk])
            kwb = dict(table=tab, seg=bk)
        for act in ACTS:
            pre = R.gemm_epilogue_ref(z, bias=bias if bk == "static" else None, table=tables.get(bk), seg_rows=bk if tab else 0)
            post = R.act_ref(pre, act)
            refs = {False: post.to(dev), True: (post + res.double()).to(dev)}
            bounds = {r: R.act_bound(pre, act, res if r else None) for r in (False, True)}
            for outs in OUTSETS:
                for rk in _residual_kinds(outs):
                    if not _defeats_vec(path, outs, rk):
                        continue
                    what = f"gemm16 {dtype} tile {tile} {path} outs={'+'.join(outs)} bias={bk} act={act} residual={rk}"

                    def run(generic=False):
                        c32 = _Win(dev, "f32", M, N, ld32, data=res_d if rk == "inplace" else None) if "c32" in outs else None
                        c16 = _Win(dev, dtype, M, N, ld16, off=off16) if "c16" in outs else None
                        lo = _Win(dev, dtype, M, N, ld16) if "lo" in outs else None
                        rw = c32 if rk == "inplace" else (_Win(dev, "f32", M, N, ldr, data=res_d) if rk == "separate" else None)
                        with _option("gemm_generic_epi", 1 if generic else 0):
                            _launch(P, M, N, K, dtype, passes, tile, c32=c32, c16=c16, lo=lo, residual=rw, act=act, **kwb)
                        return c32, c16, lo, rw
                    c32, c16, lo, rw = run()
                    n_launch += 1
                    ref = refs[rk != "absent"]
                    bound, model = bounds[rk != "absent"]
                    if c32 is not None:
                        _assert32(c32, ref, bound, what, model)
                    if c16 is not None:
                        _assert16(c16.view, lo.view if lo else None, ref, dtype, what)
                        assert c16.untouched_outside() and (lo is None or lo.untouched_outside()), f"{what}: 16-bit plane written outside its window"
                        if c32 is not None:
                            _assert_planes_of(c32.view, c16.view, lo.view if lo else None, dtype, what)
                    if rk == "separate":
                        assert torch.equal(rw.view, res_d) and rw.untouched_outside(), f"{what}: the residual was written"
                    if tab is not None:
                        assert tab.untouched_outside(), f"{what}: the bias table's buffer was written"
                    if path == "vec" and len(outs) == 1:          # {c32}: epilogue32, {c16}: epilogue_pk, where the host selects them
                        g32, g16, _, _ = run(generic=True)
                        got, want = (c32, g32) if c32 is not None else (c16, g16)
                        assert torch.equal(got.view, want.view), f"{what}: the specialised epilogue differs from the generic one"
    assert n_launch >= 100


# ------------------------------------------------------------------------------------------------------ C4. head-major output
def _to_hm(x, B, T, W, H):
    """[B*T, W*H*64] -> flat [W][B][H][T][64] (R.to_headmajor for any number W of q | k | v blocks)."""
    out = x.reshape(B, T, W, H, 64).permute(2, 0, 3, 1, 4).contiguous()
    if W == 3:
        assert torch.equal(out, R.to_headmajor(x.contiguous(), B, T, H))
    return out.reshape(1, -1)


def _hm_cases():
    cases = []
    for dtype in DTYPES:
        for T in (1, 50):
            for tile, H, W in ((2, 1, 1), (1, 1, 3), (1, 2, 3), (3, 1, 3), (3, 2, 3)):
                for with_lo in (False, True):
                    B = 3 if (H + T + with_lo) % 2 else 2
                    cases.append(pytest.param(dtype, tile, H, W, T, B, with_lo, id=f"{dtype}-t{tile}-H{H}-T{T}-B{B}-{'lo' if with_lo else 'hi'}"))
    return cases


@pytest.mark.parametrize("dtype,tile,H,W,T,B,with_lo", _hm_cases())
def test_headmajor_output(dev, dtype, tile, H, W, T, B, with_lo):
    """headmajor_T / headmajor_H: the planes hold R.to_headmajor of the row-major result — against fp64 and, bit for bit, against the
    row-major launch.  Then the same call with vec_ok defeated (ldc16 = N + 4; a c32 with ldc32 = N + 1): the library must write the
    same head-major planes or refuse with MER_ESHAPE before it launches.  It refuses: the scalar epilogue of csrc/gemm16_impl.h has
    no scatter (it would store row-major at row * ldc16 + col, past the planes), so mer_gemm16 requires the vector epilogue."""
    M, N, K = B * T, W * H * 64, 64
    P = _Planes(dev, M, N, K, dtype, seed=2)
    bias = R.rand((N,), 9201)
    ref = R.gemm_epilogue_ref(P.ref(1), bias=bias).to(dev)
    bias_d = bias.to(dev)
    layout = functools.partial(_to_hm, B=B, T=T, W=W, H=H)
    what = f"head-major gemm16 {dtype} tile {tile} B={B} T={T} H={H} which={W} lo={with_lo}"

    def planes():
        return _Win(dev, dtype, 1, M * N, M * N), (_Win(dev, dtype, 1, M * N, M * N) if with_lo else None)
    hm, hml = planes()
    _launch(P, M, N, K, dtype, 1, tile, c16=hm, lo=hml, bias=bias_d, headmajor=(T, H), ldc16=N)
    rm, rml = _Win(dev, dtype, M, N, N + 8), (_Win(dev, dtype, M, N, N + 8) if with_lo else None)
    _launch(P, M, N, K, dtype, 1, tile, c16=rm, lo=rml, bias=bias_d)
    torch.cuda.synchronize()
    _assert16(hm.view, hml.view if with_lo else None, ref, dtype, what, layout)
    assert hm.untouched_outside() and (hml is None or hml.untouched_outside()), f"{what}: written outside the head-major planes"
    assert torch.equal(hm.view, layout(rm.view)) and (not with_lo or torch.equal(hml.view, layout(rml.view))), f"{what}: != row-major launch"
    # vec_ok defeated two ways: correct head-major planes, or MER_ESHAPE and nothing written
    for how in ("ldc16", "ldc32"):
        hm2, hml2 = planes()
        c32 = _Win(dev, "f32", M, N, N + 1) if how == "ldc32" else None
        g = _args(P, M, N, K, dtype, 1, tile, c32=c32, c16=hm2, lo=hml2, bias=bias_d, headmajor=(T, H), ldc16=N + 4 if how == "ldc16" else N)
        rc = _lib().mer_gemm16(g, _ops().stream())
        torch.cuda.synchronize()
        if rc == 0:      # (the contract's other half: mer_gemm16 refuses today, so only the else branch is reachable)
            assert torch.equal(hm2.view, hm.view) and (not with_lo or torch.equal(hml2.view, hml.view)), f"{what}: wrong planes with {how} defeating vec_ok"
            assert hm2.untouched_outside() and (hml2 is None or hml2.untouched_outside())
        else:
            assert rc == MER_ESHAPE, f"{what}: rc {rc} with {how} defeating vec_ok"
            assert hm2.untouched() and (hml2 is None or hml2.untouched()) and (c32 is None or c32.untouched()), f"{what}: refused but wrote"


def test_headmajor_needs_the_vector_epilogue(dev):
    """Pins the refusal itself: a head-major launch whose outputs cannot take 16-byte accesses is MER_ESHAPE and writes nothing, for
    each of the four ways the host can lose vec_ok; the aligned launch of the same arguments is accepted."""
    dtype, tile, B, T, H = "f16", 1, 2, 50, 1
    M, N, K = B * T, 3 * H * 64, 64
    P = _Planes(dev, M, N, K, dtype, seed=2)
    res = R.rand((M, N), 9301)
    for how in ("ok", "ldc16", "c16_hi pointer", "ldc32", "ldr"):
        hm = _Win(dev, dtype, 1, M * N + 8, M * N + 8, off=1 if how == "c16_hi pointer" else 0)
        c32 = _Win(dev, "f32", M, N, N + 1 if how == "ldc32" else N + 4)
        rw = _Win(dev, "f32", M, N, N + 1 if how == "ldr" else N + 4, data=res)
        g = _args(P, M, N, K, dtype, 1, tile, c32=c32, c16=hm, residual=rw, headmajor=(T, H), ldc16=N + 4 if how == "ldc16" else N)
        rc = _lib().mer_gemm16(g, _ops().stream())
        torch.cuda.synchronize()
        assert rc == (0 if how == "ok" else MER_ESHAPE), f"head-major launch, {how}: rc {rc}"
        if how != "ok":
            assert hm.untouched() and c32.untouched(), f"{how}: refused but wrote"


# ---------------------------------------------------------------------------------------------------- C5. batched launches
@pytest.mark.parametrize("path", ["vec", "scalar"])
@pytest.mark.parametrize("passes", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile", sorted(TILE_DIMS))
def test_batched_launch(dev, tile, dtype, passes, path):
    """nbatch = 6, nb_inner = 3 with six distinct strides; the outputs of the three inner batches interleave in the columns of one
    buffer (as the grouped positional conv writes them) with canary columns between them and canary rows between the outer batches.
    vec: c_si % 8 == 0; scalar: c_si = 12 (then N = 8: the slices must not overlap)."""
    BM, BN = TILE_DIMS[tile]
    NO, NI, K = 2, 3, 64
    M = BM + 1
    N, c_si = (BN + 8, BN + 16) if path == "vec" else (8, 12)
    ldc = NI * c_si + (8 if path == "vec" else 4)
    c_so = (M + 1) * ldc if path == "vec" else (M + 1) * ldc + 4
    t16 = R.T16[dtype]
    lda, ldw = K + 8, K
    a_si, w_si, bias_si = (M + 2) * lda, (N + 1) * ldw, N + 8
    a_so = NI * a_si + 8 * lda

    A = [torch.full((NO * a_so,), float("nan"), dtype=t16) for _ in range(2)]
    Wt = [torch.full((NI * w_si,), float("nan"), dtype=t16) for _ in range(2)]
    bias = torch.full((NI * bias_si,), float("nan"))
    ref = {}
    for zi in range(NI):
        _, _, wh, wl = R.indep_planes(1, N, K, dtype, 9400 + 10 * zi)
        for buf, src in zip(Wt, (wh, wl)):
            torch.as_strided(buf, (N, K), (ldw, 1), zi * w_si).copy_(src)
        b = R.rand((N,), 9450 + zi)
        bias[zi * bias_si: zi * bias_si + N] = b
        for zo in range(NO):
            ah, al, _, _ = R.indep_planes(M, 1, K, dtype, 9500 + 10 * zi + 100 * zo)
            for buf, src in zip(A, (ah, al)):
                torch.as_strided(buf, (M, K), (lda, 1), zo * a_so + zi * a_si).copy_(src)
            ref[zo, zi] = R.gemm_epilogue_ref(R.gemm16_planes_ref(ah, al, wh, wl, passes), bias=b, act="gelu")
    Ad, Wd, bias_d = [t.to(dev) for t in A], [t.to(dev) for t in Wt], bias.to(dev)
    P = types.SimpleNamespace()
    P.a_hi, P.a_lo = [torch.as_strided(t, (M, K), (lda, 1), 0) for t in Ad]
    P.w_hi, P.w_lo = [torch.as_strided(t, (N, K), (ldw, 1), 0) for t in Wd]
    rows, cols = (NO - 1) * c_so // ldc + M + 2, ldc                       # one [rows, ldc] buffer per output kind holds every slice
    span = (NO - 1) * c_so + (NI - 1) * c_si + (M - 1) * ldc + N
    assert span <= rows * cols

    def slices(win):
        return {(zo, zi): torch.as_strided(win.flat, (M, N), (ldc, 1), win.start + zo * c_so + zi * c_si) for zo in range(NO) for zi in range(NI)}

    def untouched_between(win, fill):
        c = win.flat.clone().view(torch.int16 if win.kind != "f32" else torch.float32)
        for zo in range(NO):
            for zi in range(NI):
                torch.as_strided(c, (M, N), (ldc, 1), win.start + zo * c_so + zi * c_si).fill_(fill)
        return bool((c == fill).all())
    kw = dict(nbatch=NO * NI, nb_inner=NI, a_so=a_so, a_si=a_si, w_si=w_si, bias_si=bias_si, c_so=c_so, c_si=c_si)
    both32, both16, only16 = _Win(dev, "f32", rows, cols, cols), _Win(dev, dtype, rows, cols, cols), _Win(dev, dtype, rows, cols, cols)
    _launch(P, M, N, K, dtype, passes, tile, c32=both32, c16=both16, bias=bias_d, act="gelu", ldc32=ldc, ldc16=ldc, **kw)   # generic epilogue
    _launch(P, M, N, K, dtype, passes, tile, c16=only16, bias=bias_d, act="gelu", ldc16=ldc, **kw)                          # packed-pair on the vector path
    torch.cuda.synchronize()
    what = f"batched gemm16 {dtype} tile {tile} passes {passes} {path}"
    assert untouched_between(both32, R.CANARY32) and untouched_between(both16, 0x7B7B) and untouched_between(only16, 0x7B7B), \
        f"{what}: written between the slices"
    s32, s16, p16 = slices(both32), slices(both16), slices(only16)
    for key, r in ref.items():
        r = r.to(dev)
        e = _err32(s32[key], r)
        assert bool(torch.isfinite(s32[key]).all()) and e <= R.GEMM_TOL, f"{what} batch {key}: c32 err {e:.3e} > {R.GEMM_TOL:.1e}"
        _assert16(s16[key], None, r, dtype, f"{what} batch {key}")
        _assert_planes_of(s32[key], s16[key], None, dtype, f"{what} batch {key}")
        assert torch.equal(p16[key], s16[key]), f"{what} batch {key}: 16-bit-only launch differs from the fp32 + 16-bit one"


# --------------------------------------------------------------------------------------------------- C6. implicit-conv rows
@pytest.mark.parametrize("C,k", [(16, 3), (32, 2)])                       # K = 48: register-staged loader; K = 64: LDS-DMA
@pytest.mark.parametrize("passes", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile", sorted(TILE_DIMS))
def test_implicit_conv_rows(dev, tile, dtype, passes, C, k):
    """a_rows_per_batch / a_batch_stride / lda = s C: overlapping windows of a channels-last [B, Tin, C] plane as GEMM rows; Tout = 100
    is no multiple of a tile height, so a tile's rows cross from one clip into the next."""
    BM, BN = TILE_DIMS[tile]
    B, Tout, s = 3, 100, 2
    Tin, K, M, N = (Tout - 1) * s + k, k * C, B * Tout, BN + 8
    assert M > BM and any((b * Tout) % BM for b in range(1, B))
    xh, xl, _, _ = R.indep_planes(B * Tin, 1, C, dtype, 9600)
    _, _, wh, wl = R.indep_planes(1, N, K, dtype, 9610)
    win = [x.view(B, Tin, C).unfold(1, k, s).permute(0, 1, 3, 2).reshape(B * Tout, K) for x in (xh, xl)]    # (kk, ci) order
    ref = R.gemm16_planes_ref(win[0], win[1], wh, wl, passes).to(dev)
    P = types.SimpleNamespace()
    tail = torch.full((8,), float("nan"), dtype=xh.dtype)                    # the last window ends with the plane: NaN right behind it
    P.a_hi, P.a_lo = [torch.cat([x.reshape(-1), tail]).to(dev)[:B * Tin * C].view(B * Tin, C) for x in (xh, xl)]
    P.w_hi, P.w_lo = _padded(wh, 16, dev), _padded(wl, 16, dev)
    wins = [_Win(dev, "f32", M, N, N + 8) for _ in range(2)]
    for w in wins:
        _launch(P, M, N, K, dtype, passes, tile, c32=w, lda=s * C, a_rows_per_batch=Tout, a_batch_stride=Tin * C)
    torch.cuda.synchronize()
    what = f"implicit conv gemm16 {dtype} tile {tile} passes {passes} C={C} k={k}"
    _assert32(wins[0], ref, R.GEMM_TOL, what)
    assert torch.equal(wins[0].view, wins[1].view) and wins[1].untouched_outside(), f"{what}: two launches differ"


# ------------------------------------------------------------------------------------------------------------ D. auto tile
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,passes", [(300, 64, 1), (300, 65, 1), (1023, 1280, 1), (1024, 1280, 1), (1024, 191, 1), (1024, 192, 1),
                                        (1024, 1024, 1), (1024, 1032, 1), (1024, 191, 4), (1024, 192, 4)])
def test_auto_tile_rule(dev, dtype, M, N, passes):
    """tile = 0 at the edges of the rule in mer_gemm16 (R.auto_tile): bit-equal to the launch with that tile forced, and within the
    bound of fp64.  Not seen here (module docstring): WHICH tile ran — all three give the same bits and the launch profiler's labels
    are per pass set; the rule itself is pinned only as R.auto_tile, on the CPU.  passes 4 without an MX plane runs the 2-pass kernels and is the one launch that is never `few_narrow`: the only
    way to the N >= 192 edge below 24577 rows."""
    K = 32
    want = R.auto_tile(M, N, passes)
    assert want == {(300, 64): 2, (300, 65): 1, (1023, 1280): 1, (1024, 1280): 3, (1024, 1024): 1, (1024, 1032): 3}.get(
        (M, N), 3 if (N, passes) == (192, 4) else 1)
    P = _Planes(dev, M, N, K, dtype, seed=3)
    auto, forced = _Win(dev, "f32", M, N, _ld32(N)), _Win(dev, "f32", M, N, _ld32(N))
    _launch(P, M, N, K, dtype, passes, 0, c32=auto)
    _launch(P, M, N, K, dtype, 2 if passes == 4 else passes, want, c32=forced)
    torch.cuda.synchronize()
    what = f"gemm16 {dtype} ({M}, {N}, {K}) passes {passes} tile 0 (rule: {want})"
    _assert32(auto, P.ref(2 if passes == 4 else passes).to(dev), R.GEMM_TOL, what)
    assert forced.untouched_outside() and torch.equal(auto.view, forced.view), f"{what}: differs from the forced tile"


# --------------------------------------------------------------------------------------- E. persistent kernel at its smallest
P_M = (1, 191, 192, 193, 255, 256, 257, 513)
# (outputs, act, bias kind, residual kind): every bias kind under the 16-bit, the fp32 and the fp32 + residual epilogue; every
# activation the 16-bit epilogue may take; 39 rows per sequence is below the persistent kernel's 40: the host keeps the tile kernel
P_EPI = [("c16", None, "none", "absent"), ("c16", "gelu", "static", "absent"), ("c16", "quick_gelu", 40, "absent"),
         ("c16", "gelu_tanh", 41, "absent"), ("c16", None, 39, "absent"),
         ("c32", None, "static", "absent"), ("c32", "gelu", 40, "absent"), ("c32", None, "none", "absent"), ("c32", "gelu", 39, "absent"),
         ("c32", None, "static", "separate"), ("c32", None, 41, "separate"), ("c32", None, 39, "separate"),
         ("c32", None, 40, "inplace"), ("c32", None, "none", "inplace")]


@pytest.mark.parametrize("K", [256, 288])                                 # 8 slabs (the minimum) and an odd count, 9
@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("tm", [3, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_persistent_smallest(dev, dtype, tm, N, K):
    """gemm16p_kernel through dispatch_p at both tile heights on one to six tiles: bit-equal to the tile kernel (gemm_persist = 0) on
    strided, canaried outputs, within the bounds of the fp64 plane reference, and the same bits on a second launch.  The profiler's
    label shows that the persistent kernel ran, not at which height: gemm_tm is taken on trust (both heights give the same bits)."""
    ops = _ops()
    Mmax = max(P_M)
    P = _Planes(dev, Mmax, N, K, dtype, seed=4)
    wh = P.w_hi.contiguous()
    hb, hp, hq = ops.w_block_pack(wh), ops.w_block_pack_p(wh, 0), ops.w_block_pack_p(wh, 1)
    assert hb is not None and hp is not None and hq is not None
    blk = dict(w_hi_blk=hb.data_ptr(), w_hi_blkp=hp.data_ptr(), w_hi_blkq=hq.data_ptr())
    zfull = P.ref(1)
    bias, res = R.rand((N,), 9701), R.rand((Mmax, N), 9702)
    bias_d = bias.to(dev)
    for M in P_M:
        z = zfull[:M]
        for out, act, bk, rk in P_EPI:
            what = f"persistent gemm16 {dtype} {64 * tm}-row tiles ({M}, {N}, {K}) {out} act={act} bias={bk} residual={rk}"
            tab_cpu = R.rand(((M + bk - 1) // bk, N), 9800 + bk) if isinstance(bk, int) else None
            pre = R.gemm_epilogue_ref(z, bias=bias if bk == "static" else None, table=tab_cpu, seg_rows=bk if tab_cpu is not None else 0)
            ref = R.act_ref(pre, act)
            r_cpu = res[:M] if rk != "absent" else None
            bound, model = R.act_bound(pre, act, r_cpu)
            if r_cpu is not None:
                ref = ref + r_cpu.double()
            ref = ref.to(dev)

            def run():
                kwb = {}
                tab = None
                if tab_cpu is not None:
                    tab = _Win(dev, "f32", tab_cpu.shape[0], N, N + 8, data=tab_cpu)
                    kwb = dict(table=tab, seg=bk)
                elif bk == "static":
                    kwb = dict(bias=bias_d)
                c32 = _Win(dev, "f32", M, N, N + 8, data=r_cpu if rk == "inplace" else None) if out == "c32" else None
                c16 = _Win(dev, dtype, M, N, N + 8) if out == "c16" else None
                rw = c32 if rk == "inplace" else (_Win(dev, "f32", M, N, N + 8, data=r_cpu) if rk == "separate" else None)
                _launch(P, M, N, K, dtype, 1, 3, c32=c32, c16=c16, residual=rw, act=act, **kwb, **blk)
                return (c32 if c32 is not None else c16), rw, tab
            got = []
            with _option("gemm_tm", tm):
                labels = _profiled(lambda: got.extend([run(), run()]))
            with _option("gemm_persist", 0):
                want = run()
            torch.cuda.synchronize()
            assert labels == ({"gemm16": 2} if bk == 39 else {"gemm16p": 2}), f"{what}: launched {labels}"
            (o1, rw, tab), (o2, _, _) = got
            assert torch.equal(o1.view, want[0].view), f"{what}: differs from the tile kernel"
            assert torch.equal(o1.view, o2.view), f"{what}: two launches differ"
            for o in (o1, o2):
                assert o.untouched_outside(), f"{what}: written outside the [M, N] window"
            if rk == "separate":
                assert torch.equal(rw.view, r_cpu.to(dev)) and rw.untouched_outside(), f"{what}: the residual was written"
            if tab is not None:
                assert tab.untouched_outside(), f"{what}: the bias table's buffer was written"
            if out == "c32":
                _assert32(o1, ref, bound, what, model)
            else:
                _assert16(o1.view, None, ref, dtype, what)
