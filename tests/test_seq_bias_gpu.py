"""mer_seq_bias (csrc/norm.hip: seqmean16_kernel + seqbias_kernel) at its sampling, slicing and tile edges (GPU).

The call goes through the C ABI (_Call below): ops.seq_bias cannot express lda, ldt, a_rows_per_batch / a_batch_stride or hand
back the scratch, and the 16-bit mean plane [nseq, K] in the scratch is the first intermediate under test.

What is compared with what (references and bounds: tests/op_refs.py, pinned on the CPU in tests/test_op_refs_cpu.py):
  mean plane   torch.equal to R.seq_mean16_ref, the integer model restated from the words of include/mer_hip.h — no tolerance —
               and, separately, the header's plain statement |mean16 - fp64 mean of the samples| <= 2^-15 + one rounding
  table        within R.seq_bias_bound (counted roundings, elementwise) of R.seq_bias_table_ref ON THE MEAN PLANE READ BACK, with a
               w_lo of order 1 (to the kernel it is a 16-bit plane like any other): a dropped 32-wide k-step is hundreds of bounds
               out (test_op_refs_cpu.py); columns below n_first are the bias bit for bit
  reads        the A buffer is NaN wherever the contract does not read: rows that are no sample, rows at and above the valid length,
               rows past M, columns K .. lda, the padding between batches; w_lo is NaN in columns K .. ldw and in the rows around
               it.  A NaN that is read counts as -131000 in a mean: the plane then differs from the model
  writes       the table is a window (ldt > N) of a canary buffer with rows in front and behind, the scratch is followed by a
               canary from the first byte after the mean plane; A, w_lo, bias and valid_rows are compared with their copies

Nothing here is a measured tolerance.
"""
import functools

import pytest
import torch

import op_refs as R

pytestmark = pytest.mark.gpu

DTYPES = ("f16", "bf16")
MER_EINVAL, MER_ESHAPE, MER_EUNSUPPORTED = -1, -2, -5
SEG_ROWS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 127, 128, 255, 256, 511)
MEAN_K = (8, 504, 512, 520, 1032)                      # the 512-column slices of seqmean16_kernel and their partial tails
LAYOUTS = ("dense", "lda+8", "lda2k", "batch1", "batch3")
SCRATCH_CANARY = 0x5A


def _mods():
    from mertools_amd import _lib, ops
    return _lib, ops


def _layout(kind, T, K):
    """-> (lda, a_rows_per_batch, a_batch_stride).  "lda2k": the stride-2 rows of an implicit-conv A plane; "batch1": seg_rows == rows
    per batch, "batch3": seg_rows divides it; both with 24 elements of padding between the batches."""
    if kind == "dense":
        return K, 0, 0
    if kind == "lda+8":
        return K + 8, 0, 0
    if kind == "lda2k":
        return 2 * K, 0, 0
    rpb = T if kind == "batch1" else 3 * T
    lda = K + 8 if kind == "batch1" else 2 * K
    return lda, rpb, rpb * lda + 24


class _Call:
    """One mer_seq_bias launch on buffers that make every stray read or write visible.  a: logical 16-bit plane [M, K] on the CPU
    (what the reference sees); only the elements the contract reads reach the device buffer, the rest of it is NaN."""

    def __init__(self, dev, a, dtype, seg_rows, w_lo, *, valid=None, bias=None, n_first=0, layout="dense", ldw_extra=0, ldt_extra=5,
                 nan_unread=True):
        _lib, ops = _mods()
        self.dtype, self.T = dtype, seg_rows
        M, K = a.shape
        N = w_lo.shape[0]
        self.M, self.K, self.N = M, K, N
        self.nseq = nseq = -(-M // seg_rows)
        lda, rpb, bstride = _layout(layout, seg_rows, K)
        self.lda, self.rpb, self.bstride = lda, rpb, bstride
        off = (lambda r: (r // rpb) * bstride + (r % rpb) * lda) if rpb else (lambda r: r * lda)
        rows_buf = nseq * seg_rows + 2                                     # the rows past M exist, as NaN
        abuf = torch.full((off(rows_buf) + lda,), float("nan"), dtype=a.dtype)
        read = range(M)
        if nan_unread:
            read = [s * seg_rows + r for s in range(nseq)
                    for r in R.seq_sample_rows(seg_rows, seg_rows if valid is None else int(valid[s]), M - s * seg_rows)]
        for r in read:
            abuf[off(r):off(r) + K] = a[r]
        self.a_dev = abuf.to(dev)
        ldw = K + ldw_extra
        wbuf = torch.full((N + 2, ldw), float("nan"), dtype=w_lo.dtype)
        wbuf[1:N + 1, :K] = w_lo
        self.w_dev = wbuf.to(dev)
        self.ldw = ldw
        self.bias_dev = None if bias is None else bias.to(dev)
        self.valid_dev = None if valid is None else torch.as_tensor(valid, dtype=torch.int32).to(dev)
        self.n_first = n_first
        self.ldt = ldt = N + ldt_extra
        self.tab_flat = R.canary32(((nseq + 5) * ldt,), dev)
        self.table = torch.as_strided(self.tab_flat, (nseq, N), (ldt, 1), 2 * ldt)
        nbytes = int(_lib.lib().mer_seq_bias_scratch_bytes(nseq, K))
        assert nbytes >= nseq * K * 2 and nbytes % 256 == 0
        self.scratch = torch.full((nbytes + 256,), SCRATCH_CANARY, dtype=torch.uint8, device=dev)
        self.inputs = [t for t in (self.a_dev, self.w_dev, self.bias_dev, self.valid_dev) if t is not None]
        self.before = [t.clone() for t in self.inputs]

    def run(self, **over):
        _lib, ops = _mods()
        p = dict(a=self.a_dev.data_ptr(), dtype=ops.dt_code(self.dtype), lda=self.lda, rpb=self.rpb, bstride=self.bstride, M=self.M, K=self.K,
                 T=self.T, valid=None if self.valid_dev is None else self.valid_dev.data_ptr(), w=self.w_dev[1:].data_ptr(), ldw=self.ldw,
                 bias=None if self.bias_dev is None else self.bias_dev.data_ptr(), N=self.N, n_first=self.n_first,
                 scratch=self.scratch.data_ptr(), table=self.table.data_ptr(), ldt=self.ldt)
        p.update(over)
        return _lib.lib().mer_seq_bias(p["a"], p["dtype"], p["lda"], p["rpb"], p["bstride"], p["M"], p["K"], p["T"], p["valid"], p["w"], p["ldw"],
                                       p["bias"], p["N"], p["n_first"], p["scratch"], p["table"], p["ldt"], ops.stream())

    def mean16(self):
        return self.scratch[:self.nseq * self.K * 2].view(R.T16[self.dtype]).view(self.nseq, self.K)

    def table_untouched(self):
        return R.is_canary32(self.tab_flat)

    def scratch_untouched(self):
        return bool((self.scratch == SCRATCH_CANARY).all())

    def assert_clean(self, what):
        """Nothing but the table window and the mean plane changed."""
        c = self.tab_flat.clone()
        torch.as_strided(c, (self.nseq, self.N), (self.ldt, 1), 2 * self.ldt).fill_(R.CANARY32)
        assert R.is_canary32(c), f"{what}: table written outside its [nseq, N] window (ldt {self.ldt})"
        assert bool((self.scratch[self.nseq * self.K * 2:] == SCRATCH_CANARY).all()), f"{what}: scratch written past the mean plane"
        for t, b in zip(self.inputs, self.before):
            assert torch.equal(t.view(torch.uint8), b.view(torch.uint8)), f"{what}: an input buffer changed"


def _bits(t):
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t.contiguous().view(torch.int32)


def _assert_mean(call, a, valid, what):
    got = call.mean16().cpu()
    want = R.seq_mean16_ref(a, call.T, valid)
    if not torch.equal(_bits(got), _bits(want)):
        bad = (_bits(got) != _bits(want)).nonzero()
        s, k = bad[0].tolist()
        raise AssertionError(f"{what}: mean plane differs from the integer model in {len(bad)} elements, first at sequence {s} column {k}: "
                             f"{got[s, k].item()!r} != {want[s, k].item()!r}")
    return got


def _assert_table(call, mean16, w_lo, bias, what):
    ref = R.seq_bias_table_ref(mean16, w_lo, bias, call.n_first)
    bound = R.seq_bias_bound(mean16, w_lo, bias, call.n_first)
    tab = call.table.cpu()
    assert bool(torch.isfinite(tab).all()), f"{what}: non-finite table"
    ratio = R.worst_ratio(tab, ref, bound)
    print(f"{what}: table error / bound {ratio:.3g}")
    assert ratio <= 1.0, f"{what}: table is {ratio:.3g} x seq_bias_bound from the fp64 product on the mean plane"
    nf = min(call.n_first, call.N)
    plain = torch.zeros((call.nseq, nf)) if bias is None else bias[None, :nf].expand(call.nseq, -1)
    assert torch.equal(tab[:, :nf], plain), f"{what}: a column below n_first is not the plain bias"


# ----------------------------------------------------------------------------------------------------------- A. the mean plane
def _mean_valid(T):
    s = R.seq_sample_stride(T)
    h = s // 2
    return [0, h, h + 1, h + s, h + s + 1, T - 1, T, T + 5]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", SEG_ROWS)
def test_mean_plane_is_the_integer_model(dev, dtype, T):
    """Eight sequences at the eight valid_rows values around the first two samples and the end, then a last, partial sequence with 1,
    h, h + 1 and T - 1 rows left; once more without valid_rows.  K and the A layout rotate with (T, dtype) so that every K and every
    layout meets both dtypes; the table rides along (N = 17, order-1 w_lo) and is held to its bound."""
    i = SEG_ROWS.index(T) + DTYPES.index(dtype)
    K, layout = MEAN_K[i % len(MEAN_K)], LAYOUTS[(i // 2) % len(LAYOUTS)]
    s = R.seq_sample_stride(T)
    h = s // 2
    N = 17
    a_full = R.seq_grid_values((9 * T, K), 100 + T, dtype)
    w_lo = R.rand((N, K), 200 + T).to(R.T16[dtype])
    bias = R.rand((N,), 300 + T)
    lefts = sorted({1, h, h + 1, T - 1} - {0}) or [0]
    runs = []
    for left in lefts:
        M = 8 * T + left
        valid = (_mean_valid(T) + [T])[:-(-M // T)]
        runs.append((M, valid, f"rows_left={left}"))
    runs.append((8 * T + lefts[-1], None, "no valid_rows"))
    calls = []
    for M, valid, tag in runs:
        c = _Call(dev, a_full[:M], dtype, T, w_lo, valid=valid, bias=bias, layout=layout, ldw_extra=8)
        assert c.run() == 0, tag
        calls.append(c)
    torch.cuda.synchronize()
    for c, (M, valid, tag) in zip(calls, runs):
        what = f"seq_bias {dtype} T={T} K={K} {layout} {tag}"
        mean16 = _assert_mean(c, a_full[:M], valid, what)
        m64 = R.seq_sample_mean64(a_full[:M], T, valid)
        r = R.worst_ratio(mean16, m64, R.seq_mean16_plain_bound(m64, dtype))
        assert r <= 1.0, f"{what}: mean16 is {r:.3g} x (2^-15 + one rounding) from the fp64 mean of the samples"
        _assert_table(c, mean16, w_lo, bias, what)
        c.assert_clean(what)


def test_mean_plane_cases_cover_the_axes():
    """(no GPU work) the rotation of test_mean_plane_is_the_integer_model reaches every K and layout with both dtypes, and the
    sample counts 31 (T = 63) and 32 (T = 127, 255, 511) occur."""
    seen = {(d, MEAN_K[(i + j) % 5]) for i, _ in enumerate(SEG_ROWS) for j, d in enumerate(DTYPES)}
    assert seen == {(d, k) for d in DTYPES for k in MEAN_K}
    lay = {(d, LAYOUTS[((i + j) // 2) % 5]) for i, _ in enumerate(SEG_ROWS) for j, d in enumerate(DTYPES)}
    assert lay == {(d, l) for d in DTYPES for l in LAYOUTS}
    n = {T: len(R.seq_sample_rows(T, T, T)) for T in SEG_ROWS}
    assert n[63] == 31 and n[127] == n[255] == n[511] == 32 and n[16] == 16 and n[17] == 17 and n[15] == 15
    assert {R.seq_sample_stride(T) for T in SEG_ROWS} == {1, 2, 4, 8, 16}


def test_clamp_and_non_finite_samples(dev):
    """bf16 samples of 2^17 and 2^20 count as 131000; +inf counts as 131000, -inf and a NaN in a sampled row as -131000 (the header's
    words).  The means stay finite."""
    T, K = 16, 8
    a = R.seq_grid_values((3 * T, K), 7, "bf16")
    a[:T, 0] = 2.0 ** 17
    a[:T:2, 1] = 2.0 ** 20
    a[:T:2, 2] = -(2.0 ** 20)
    a[T + 3, 4] = float("inf")
    a[T + 5, 5] = float("-inf")
    a[2 * T + 7, 6] = float("nan")
    w_lo = R.rand((16, K), 8).bfloat16()
    c = _Call(dev, a, "bf16", T, w_lo)
    assert c.run() == 0
    torch.cuda.synchronize()
    m = _assert_mean(c, a, None, "clamp / non-finite").double()
    assert bool(torch.isfinite(m).all())
    b = lambda x: torch.tensor(x).bfloat16().item()      # noqa: E731
    assert m[0, 0].item() == b(131000.0) and m[0, 1].item() > 65000.0 and m[0, 2].item() < -65000.0
    rest = a[T:2 * T, 4].double()
    assert m[1, 4].item() == b(float(((rest[rest.isfinite()] * 16384).round().sum() + 131000.0 * 16384) / (16 * 16384.0)))
    assert m[1, 5].item() < -8000.0 and m[2, 6].item() < -8000.0
    _assert_table(c, c.mean16().cpu(), w_lo, None, "clamp / non-finite")
    c.assert_clean("clamp / non-finite")


# ---------------------------------------------------------------------------------------------------------------- B. the table
# (K, N, n_first, nseq, bias): every value of every axis of the issue occurs; nseq = 40 adds mts = 3, which the listed ones skip
TABLE_CASES = ((8, 1, 0, 1, True), (24, 15, 0, 15, False), (32, 16, 0, 16, True), (40, 17, 16, 17, True), (512, 40, 32, 63, True),
               (544, 40, 48, 64, True), (2080, 40, 16, 65, False), (544, 17, 0, 130, True), (2080, 16, 0, 40, True), (40, 40, 48, 130, False))


def test_table_cases_cover_the_axes():
    Ks, Ns, nfs, nss, _ = map(set, zip(*TABLE_CASES))
    assert Ks == {8, 24, 32, 40, 512, 544, 2080} and Ns == {1, 15, 16, 17, 40} and nss >= {1, 15, 16, 17, 63, 64, 65, 130}
    assert {(nf, N) for _, N, nf, _, _ in TABLE_CASES} >= {(0, 1), (16, 17), (32, 40), (48, 40)} and nfs == {0, 16, 32, 48}
    pers = {K: R.seq_ksplit(K)[0] for K in Ks}
    assert pers[512] == 1 and pers[544] == 2 and pers[2080] == 5 and pers[8] == 1              # 544: uneven, 2080: two trips of the load loop
    idle = {K: sum(lo >= hi for lo, hi in R.seq_ksplit(K)[1]) for K in Ks}
    assert idle[8] == 15 and idle[40] == 14 and idle[512] == 0 and idle[544] == 7 and idle[2080] == 3
    mts = set()
    for ns in nss:
        mts |= {min(4, -(-(ns - s0) // 16)) for s0 in range(0, ns, 64)}
    assert mts == {1, 2, 3, 4} and max(nss) > 128


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,N,n_first,nseq,with_bias", TABLE_CASES, ids=[f"K{c[0]}-N{c[1]}-nf{c[2]}-s{c[3]}" for c in TABLE_CASES])
def test_table_within_the_derived_bound(dev, dtype, K, N, n_first, nseq, with_bias):
    T = 5
    M = nseq * T - 2
    a = (R.rand((M, K), 400 + K + nseq) * 0.7 + 0.3).to(R.T16[dtype])
    w_lo = R.rand((N, K), 500 + K + N).to(R.T16[dtype])
    bias = R.rand((N,), 600 + N) if with_bias else None
    g = torch.Generator().manual_seed(nseq)
    valid = torch.randint(0, T + 2, (nseq,), generator=g).tolist()
    what = f"seq_bias {dtype} K={K} N={N} n_first={n_first} nseq={nseq} bias={with_bias}"
    runs = [_Call(dev, a, dtype, T, w_lo, valid=valid, bias=bias, n_first=n_first, layout="lda+8", ldw_extra=16) for _ in range(2)]
    for c in runs:
        assert c.run() == 0, what
    torch.cuda.synchronize()
    c = runs[0]
    mean16 = _assert_mean(c, a, valid, what)
    _assert_table(c, mean16, w_lo, bias, what)
    for r in runs:
        r.assert_clean(what)
    assert torch.equal(_bits(runs[0].table), _bits(runs[1].table)) and torch.equal(_bits(runs[0].mean16()), _bits(runs[1].mean16())), \
        f"{what}: two runs of one call differ"


# ------------------------------------------------------------------------------------------------- C. position independence
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_sequence_does_not_depend_on_its_place(dev, dtype):
    """One fixed sequence at index 0, 15, 16, 63, 64 and 129 of batches of 1, 16, 17, 64, 65 and 130 sequences (other clips, other
    valid lengths around it): its mean row and its table row are the same bits everywhere."""
    T, K, N, v = 70, 520, 40, 55
    fixed = R.seq_grid_values((T, K), 31, dtype)
    w_lo = R.rand((N, K), 32).to(R.T16[dtype])
    bias = R.rand((N,), 33)
    rows = []
    for idx, nseq in ((0, 1), (15, 16), (16, 17), (63, 64), (64, 65), (129, 130)):
        a = R.seq_grid_values((nseq * T, K), 40 + nseq, dtype)
        a[idx * T:(idx + 1) * T] = fixed
        g = torch.Generator().manual_seed(nseq)
        valid = torch.randint(0, T + 1, (nseq,), generator=g).tolist()
        valid[idx] = v
        c = _Call(dev, a, dtype, T, w_lo, valid=valid, bias=bias, n_first=16, layout="batch1" if nseq % 2 else "lda2k")
        assert c.run() == 0
        torch.cuda.synchronize()
        what = f"seq_bias {dtype} fixed sequence at {idx} of {nseq}"
        mean16 = _assert_mean(c, a, valid, what)
        _assert_table(c, mean16, w_lo, bias, what)
        c.assert_clean(what)
        rows.append((what, _bits(mean16[idx]).clone(), _bits(c.table[idx].cpu()).clone()))
    for what, m, t in rows[1:]:
        assert torch.equal(m, rows[0][1]), f"{what}: mean row differs from the sequence alone"
        assert torch.equal(t, rows[0][2]), f"{what}: table row differs from the sequence alone"


# --------------------------------------------------------------------------------------------------- D. what the table is for
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_pass_gemm_with_the_table_is_the_full_product_on_constant_sequences(dev, dtype):
    """Sequences whose valid rows all equal one vector x (multiples of 2^-7 in [2^-4, 1): on the 2^-14 grid, exact in both formats)
    have the exact mean x, so a one-pass mer_gemm16 with the table is a_hi . (w_hi + w_lo)^T + bias on the valid rows, within the
    one-pass bound (R.GEMM_TOL, max-norm) — columns below n_first = 2 N / 3 of a fused QKV width get a_hi . w_hi^T + bias.  The same
    GEMM with the plain bias misses that bound in the corrected columns (the test would otherwise prove nothing)."""
    _lib, ops = _mods()
    T, nseq, D = 37, 6, 64
    K, N, n_first = 136, 3 * D, 2 * D
    g = torch.Generator().manual_seed(51)
    x = torch.randint(8, 128, (nseq, K), generator=g).double() / 128.0
    valid = [T, 1, 20, 36, 2, 17]                                         # ragged; valid = 1 = h has no sample: its row is the plain bias
    a = (R.rand((nseq * T, K), 52) * 0.5).to(R.T16[dtype])                # rows at and above the valid length: anything finite
    for s in range(nseq):
        a[s * T:s * T + valid[s]] = x[s].to(R.T16[dtype])
    w = R.rand((N, K), 53, 0.05)
    w_hi, w_lo = R.split_planes(w, dtype)
    bias = R.rand((N,), 54, 0.1)
    c = _Call(dev, a, dtype, T, w_lo, valid=valid, bias=bias, n_first=n_first, nan_unread=False, ldt_extra=8)
    assert c.run() == 0
    torch.cuda.synchronize()
    mean16 = _assert_mean(c, a, valid, "constant sequences")
    has = torch.tensor([len(R.seq_sample_rows(T, vl, T)) > 0 for vl in valid])
    assert torch.equal(mean16[has].double(), x[has]) and not mean16[~has].any(), "the mean of equal rows is that row"
    a_dev = torch.as_strided(c.a_dev, (nseq * T, K), (c.lda, 1))
    out, _, _ = ops.gemm16(a_dev, w_hi.to(dev), bias=c.table, bias_seg_rows=T, out32=True, passes=1)
    base, _, _ = ops.gemm16(a_dev, w_hi.to(dev), bias=c.bias_dev, out32=True, passes=1)
    torch.cuda.synchronize()
    rows = torch.cat([torch.arange(s * T, s * T + valid[s]) for s in range(nseq) if has[s]])
    full = a.double() @ (w_hi.double() + w_lo.double()).T + bias.double()
    hh = a.double() @ w_hi.double().T + bias.double()
    ref = torch.cat([hh[:, :n_first], full[:, n_first:]], 1)[rows]
    e = R.max_rel(out.cpu()[rows], ref)
    e_corr = R.max_rel(out.cpu()[rows][:, n_first:], ref[:, n_first:])
    e_base = R.max_rel(base.cpu()[rows][:, n_first:], ref[:, n_first:])
    print(f"table GEMM {dtype}: err {e:.3e} (corrected columns {e_corr:.3e}); plain bias {e_base:.3e}")
    assert e <= R.GEMM_TOL and e_corr <= R.GEMM_TOL, (e, e_corr)
    assert e_base > R.GEMM_TOL, "without the table the weight residual must show"
    c.assert_clean("constant sequences")


# ------------------------------------------------------------------------------------------------------------------ E. refusals
@functools.lru_cache(maxsize=2)
def _refusal_inputs():
    T, K, N = 16, 16, 16
    return R.seq_grid_values((3 * T, K), 61, "f16"), R.rand((N, K), 62).half(), R.rand((N,), 63)


@pytest.mark.parametrize("name,over,status", [
    ("K % 8", dict(K=12), MER_ESHAPE), ("lda % 8", dict(lda=20), MER_ESHAPE), ("ldw % 8", dict(ldw=20), MER_ESHAPE),
    ("a_batch_stride % 8", dict(rpb=16, bstride=16 * 16 + 4), MER_ESHAPE),
    ("a off alignment", "a", MER_ESHAPE), ("w_lo off alignment", "w", MER_ESHAPE), ("scratch off alignment", "scratch", MER_ESHAPE),
    ("n_first = 8", dict(n_first=8), MER_EINVAL), ("ldt < N", dict(ldt=15), MER_ESHAPE), ("dtype", dict(dtype=2), MER_EINVAL)])
def test_refusals_launch_nothing(dev, name, over, status):
    a, w_lo, bias = _refusal_inputs()
    c = _Call(dev, a, "f16", 16, w_lo, bias=bias, nan_unread=False)
    if isinstance(over, str):                                             # a pointer 8 bytes (four elements) off 16-byte alignment
        base = dict(a=c.a_dev.data_ptr(), w=c.w_dev[1:].data_ptr(), scratch=c.scratch.data_ptr())[over]
        over = {over: base + 8}
    assert c.run(**over) == status, name
    torch.cuda.synchronize()
    assert c.table_untouched() and c.scratch_untouched(), f"{name}: a refused call wrote"
    assert c.run() == 0, "the same buffers are accepted without the defect"
    torch.cuda.synchronize()
    _assert_mean(c, a, None, name)


def test_65536_sequences_are_refused_and_65535_run(dev):
    K, N = 8, 16
    a = R.seq_grid_values((65536, K), 71, "f16")
    w_lo = R.rand((N, K), 72).half()
    c = _Call(dev, a, "f16", 1, w_lo, ldt_extra=0)
    assert c.run() == MER_EUNSUPPORTED
    torch.cuda.synchronize()
    assert c.table_untouched() and c.scratch_untouched()
    c = _Call(dev, a[:65535], "f16", 1, w_lo, ldt_extra=0)
    assert c.run() == 0
    torch.cuda.synchronize()
    mean16 = c.mean16().cpu()
    x = a[:65535].double().clamp(-R.SEQ_CLAMP, R.SEQ_CLAMP)               # one sample: the mean is the sample on the 2^-14 grid
    want = ((x * R.SEQ_FIX).round().to(torch.int64).double() * (1.0 / R.SEQ_FIX)).float().half()      # (an integer sum: no -0)
    assert torch.equal(_bits(mean16), _bits(want))
    _assert_table(c, mean16, w_lo, None, "65535 sequences")
    c.assert_clean("65535 sequences")
