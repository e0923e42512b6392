"""Operator tests of the gathered-row GEMM forms (A_INDEXED: logical row m of A reads physical row index[m]) through `ops.indexed_gemm`
(md_op_indexed_gemm), and of the index tables the engines hand to them (`ops.merge_index_table`, `ops.token_index_table`: the host
functions get_index_set and da3_tok_index fill their tables with). Three kinds, launched with the engines' own parameter builders
(md_engine_util.h rows_params / deconv2_params): ROWS (Depth Pro's enc_proj through the merge tables, fov_proj with the fp32 store),
ROWS_RES (the Depth-Anything-v3 stage projection: a bias and the per-image residual table res_mod = P) and PIXSHUF (the low-resolution
deconvolution into the second channel slice of `cat`).

The tables (CPU, no device): token rows laid out as the engine lays them out -- sequence s = rows [s SS, (s + 1) SS): a cls row, g g patch
rows, padding rows up to SS -- every value unique, cls and padding rows NaN. rows[table] reshaped to [B, E, E, C] must EQUAL
oracle.depth_pro_ref.merge of the same tokens as tiles in the reference's order (tile (j, i) of image b = sequence seq0 + (j steps + i) B +
b), so a wrong source tile for a halo pixel is a wrong value. Geometries: the six of GEOMETRIES (the first two are asserted to be what
md_split_geometry / md_feature_padding give at the full-size preset) and, beside them, what the same two functions give at the tiny
and small presets (window 128, g = 8: (8, 5, 1) and (8, 3, 2)), each at B = 1, 2, 3 and a nonzero seq0.

Where the bounds of the GEMM checks come from (u = 2^-24; none is taken from a GPU result; the CPU tests evaluate every reference
formula in fp32, summed k-tile by k-tile as the kernels' k-loop walks them, and must pass with under 1 % of the elements on the tie slack):

* ROWS / PIXSHUF (EPI_STORE / EPI_PIXSHUF): v = acc + bias, ONE rounding to T: 0.5 ulp_T(|ref|) with the tie slack of close_check +
  A_MFMA max|acc + bias|, A_MFMA = 2e-5 the suite's allowance for the accumulation order of exact products behind the MFMA (operands are
  exact in the operand type, `close_check.ROUND`; weights `round_w` of the decoder tests). The fp32 store (fov_proj) has no ulp_T term.
* ROWS_RES adds u |pre + res1|: res1 is exact in T and added in fp32, one rounding of the sum (as tests/test_decoder_gemm_ops.py derives it).
* Bit identity, tolerance 0: the same entry with index = NULL over a[index] gathered on the host, same tile: the same kernel, the same
  k-loop and epilogue, only the per-lane row address differs (gemm_impl.h: srcA of gemm_kernel and gemm256_kernel).
* Untouched bytes, tolerance 0: pad columns N .. ldo, channels outside [ps_coff, ps_coff + Cout), rows behind M keep the canary;
  a, index, w, res1 compare equal afterwards.
* Poison: every row of `a` no table entry names is NaN on the device; the output must be finite.

Mutants (CPU; `MUTANT_ACTIVE(mut, case, BM)` says where each is something else than the identity, the tests assert both directions; the
mutants run on UNPOISONED rows, so a rejection is a wrong value, not a NaN): `index_ignored` and `index_plus_one` (every case),
`batch0` (every image reads image 0's rows: B > 1, i.e. not the random table), `tail_clamped` (every row of the last partial M-tile of BM
rows reads index[M - 1]: M % BM > 1; BM = 64, 128, 256 all leave a partial tile at every M here), `halo_other_tile` (the first `pad`
interior rows of a tile row taken from the halo of the tile above: the merge table only), `slice_coff_zero` (ps_coff > 0), `res_row_m`
(ROWS_RES with res_mod < M), `wrap_lost` (the third term, hi x W_lo, reads lo x W_lo instead: only the three-term mode f16x2_w32).
Nothing here tells the accumulation order inside a k-tile or the k-split of the 64 x 64 kernel apart (inside A_MFMA).

Kernel forms, from gemm_last_form / gemm_last_launch and asserted per launch: a forced tile is the tile that ran, TILE_AUTO is
md_gemm_pick_tile's choice (N <= 32: 256 x 32). On the 256 x 256 tile every launch here is the one-tile-per-workgroup family with
blocks == grid == ceil(M / 256) ceil(N / 256) -- the persistent loops take dense / convolution operands only -- and the epilogue kind is:
ROWS with T out EK_STORE when N % 8 == 0 and ldo % 8 == 0 (N = 264 / 320; every 2-byte mode), EK_GENERIC for N = 132 and for f32; ROWS
with the fp32 store EK_STORE for bf16 / f16, EK_GENERIC for f16x2 and f32; ROWS_RES EK_GENERIC (res_mod > 0); PIXSHUF EK_PIXSHUF, except
f16x2 in the general form (Cout = 36), which takes EK_GENERIC; ps_fast is set for the 2-byte modes at Cout = 64 and not at Cout = 36 or
f32. The 128 x 128, 128 x 64, 64 x 64 and 256 x 32 tiles are gemm_kernel<BM, BN> with epilogue4 (family -1)."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import close_check
from close_check import A_MFMA, F16X2, F32, FP8, ROUND, rejects
from oracle import depth_pro_ref as R
from test_decoder_gemm_ops import MODES, MODE_ID, canary, gen, round_w

assert_close_in = functools.partial(close_check.assert_close_in, tag="indexed_gemm_ops")
ROWS, ROWS_RES, PIXSHUF = range(3)
T256, T128, T256x32, T128x64, T64, TAUTO = 0, 1, 2, 3, 4, 99
TILES = (T256, T128, T128x64, T64, TAUTO)
BM_OF = {T256: 256, T128: 128, T256x32: 256, T128x64: 128, T64: 64}
EK_GENERIC, EK_STORE, EK_PIXSHUF = 0, 2, 3
U = 2.0 ** -24
TAIL = 5
GEOMETRIES = [(24, 5, 3), (24, 3, 6), (8, 3, 1), (6, 3, 1), (4, 1, 0), (4, 1, 2)]   # (g, steps, pad)


def lib():
    from burn_depth_amd import _lib
    return _lib.load()


def ops():
    from burn_depth_amd import ops as o
    return o


def terms_of(mode):
    return {"w": 1, "w16": 2, "w32": 3}[mode[1]]


# ---------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------
def preset_geometries(window, g):
    """(g, steps, pad) of the two merged levels of a Depth Pro preset: md_engine.hip depth_pro_create's own calls."""
    out = []
    for size, ov in ((4 * window, 0.25), (2 * window, 0.5)):
        st, sp = C.c_int(), C.c_int()
        assert lib().md_split_geometry(size, window, C.c_float(ov), C.byref(st), C.byref(sp)) == 0
        out.append((g, sp.value, lib().md_feature_padding(window, st.value, g)))
    return out


def token_rows(nseq, g, SS, C_=3):
    """fp64 rows [nseq SS, C]: unique values on the patch rows, NaN on the cls row and the padding rows of every sequence."""
    rows = torch.arange(nseq * SS * C_, dtype=torch.float64).reshape(nseq, SS, C_) + 1.0
    rows[:, 0] = float("nan")
    rows[:, 1 + g * g:] = float("nan")
    return rows.reshape(nseq * SS, C_)


def test_full_size_geometries_are_the_first_two():
    assert preset_geometries(384, 24) == GEOMETRIES[:2]
    assert preset_geometries(128, 8) == [(8, 5, 1), (8, 3, 2)]   # the tiny and the small preset share the 128 window


@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("geo", GEOMETRIES + [(8, 5, 1), (8, 3, 2)], ids=lambda t: "g%d_steps%d_pad%d" % t)
def test_merge_table_is_the_reference_merge(geo, B):
    g, steps, pad = geo
    if g == 8:
        assert geo in preset_geometries(128, 8) or geo == (8, 3, 1)
    SS = (g * g + 1 + 3) // 4 * 4
    for seq0 in (0, 7):
        nseq = seq0 + steps * steps * B + 1   # one sequence behind the tiles: nothing may name it
        rows = token_rows(nseq, g, SS)
        table = ops().merge_index_table(B, g, steps, pad, SS, seq0).long()
        E = g if steps == 1 else steps * (g - 2 * pad) + 2 * pad
        assert table.numel() == B * E * E == lib().md_op_merge_index_table(B, g, steps, pad, SS, seq0, None, 0)
        assert table.min() >= seq0 * SS and table.max() < (nseq - 1) * SS
        assert ((table % SS >= 1) & (table % SS <= g * g)).all(), "a cls or a padding row"
        tiles = rows.reshape(nseq, SS, -1)[seq0:seq0 + steps * steps * B, 1:1 + g * g].reshape(-1, g, g, rows.shape[1]).permute(0, 3, 1, 2)
        want = R.merge(tiles, B, pad).permute(0, 2, 3, 1)
        assert want.shape == (B, E, E, rows.shape[1])
        assert torch.equal(rows[table].reshape(want.shape), want)


@pytest.mark.parametrize("B", [1, 2, 3])
def test_token_table_names_the_patch_rows(B):
    for P, SS, seq0 in ((63, 64, 0), (36, 40, 16), (576, 580, 35), (25, 28, 2)):
        table = ops().token_index_table(B, P, SS, seq0).long()
        assert table.numel() == B * P == lib().md_op_token_index_table(B, P, SS, seq0, None, 0)
        want = torch.tensor([(seq0 + b) * SS + 1 + p for b in range(B) for p in range(P)])
        assert torch.equal(table, want)
        assert ((table % SS >= 1) & (table % SS <= P)).all()


def test_table_entries_refuse_bad_geometry_and_small_buffers():
    from burn_depth_amd import _lib
    buf = (C.c_int32 * 8)()
    assert lib().md_op_merge_index_table(1, 4, 1, 0, 20, 0, buf, 8) == _lib.MD_ERR_SHAPE        # 16 entries
    assert lib().md_op_merge_index_table(1, 4, 1, 0, 16, 0, None, 0) == _lib.MD_ERR_SHAPE       # SS < 1 + g g
    assert lib().md_op_merge_index_table(1, 4, 3, 2, 20, 0, None, 0) == _lib.MD_ERR_SHAPE       # no interior
    assert lib().md_op_token_index_table(2, 4, 4, 0, None, 0) == _lib.MD_ERR_SHAPE              # SS < 1 + P
    assert lib().md_op_token_index_table(2, 5, 8, 0, buf, 8) == _lib.MD_ERR_SHAPE
    assert all(v == 0 for v in buf)


def merge_table_py(B, g, steps, pad, SS, seq0=0, halo_other=False):
    """md_engine.hip merge_source restated; halo_other: the mutant that takes the first `pad` interior rows of tile row j > 0 from the
    bottom halo of tile row j - 1 (the same image rows, another tile's tokens)."""
    ih = g - 2 * pad

    def src(Y, mutate):
        if steps == 1:
            return 0, Y
        j = 0 if Y < pad else min((Y - pad) // ih, steps - 1)
        t = Y - j * ih
        if mutate and j > 0 and t < 2 * pad:
            j, t = j - 1, t + ih
        return j, t

    E = g if steps == 1 else steps * ih + 2 * pad
    out = []
    for b in range(B):
        for Y in range(E):
            j, ty = src(Y, halo_other)
            for X in range(E):
                i, tx = src(X, False)
                out.append((seq0 + (j * steps + i) * B + b) * SS + 1 + ty * g + tx)
    return torch.tensor(out)


@functools.lru_cache(maxsize=None)
def table(name):
    """-> (index int64 [M], rows_a, B). merge: M = 392 = one full 256-row tile + 136 rows; token: M = 126; img36: the g = 6 image table at
    sequence 16 (M = 72, the 6 x 6 map of the pixel shuffle); random: repeats, neither monotone nor a permutation."""
    if name == "merge":
        return ops().merge_index_table(2, 6, 3, 1, 40).long(), 720, 2
    if name == "token":
        return ops().token_index_table(2, 63, 64).long(), 128, 2
    if name == "img36":
        return ops().token_index_table(2, 36, 40, 16).long(), 720, 2
    assert name == "random"
    return torch.randint(0, 97, (300,), generator=gen(11)), 97, 1


def test_gpu_tables_are_what_the_issue_sizes():
    idx, rows_a, _ = table("merge")
    assert idx.numel() == 392 and rows_a == 18 * 40 and torch.equal(idx, merge_table_py(2, 6, 3, 1, 40))
    assert not torch.equal(idx, merge_table_py(2, 6, 3, 1, 40, halo_other=True))
    assert table("token")[0].numel() == 126 and table("img36")[0].numel() == 72
    idx = table("random")[0]
    assert idx.numel() == 300 and idx.unique().numel() < 97 and (idx[1:] < idx[:-1]).any()   # repeats, unnamed rows, not monotone


# ---------------------------------------------------------------------------------------------
# cases, the fp64 definition, the fp32 evaluation and the mutants
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=32)
def case(kind, tname, K, N, ldo, mode, bias=True, out_f32=False, res_mod=0, f=0, hw=None, coff=0):
    prec = mode[0]
    index, rows_a, B = table(tname)
    M = index.numel()
    g = gen(kind * 100003 + K * 7 + N * 3 + ldo + prec * 11 + len(mode[1]) + M + f + coff)
    # rows behind rows_a: what a mutant that leaves the table (row m, row index + 1) reads. Not part of the device tensor.
    a = ROUND[prec](torch.randn(rows_a + M + 1, K, generator=g))
    named = torch.zeros(rows_a, dtype=torch.bool)
    named[index] = True
    a_dev = a[:rows_a].clone()
    a_dev[~named] = float("nan")
    w = round_w(torch.randn(*((K, N, f, f) if kind == PIXSHUF else (N, K)), generator=g) / K ** 0.5, mode)
    b = torch.randn(N, generator=g) if bias else None
    r1 = r1_beyond = None
    if kind == ROWS_RES:
        r1_beyond = ROUND[prec](torch.randn(M, ldo, generator=g))   # rows behind res_mod: what a launch that forgets the wrap would read
        r1 = r1_beyond[:res_mod].clone()
    if kind == PIXSHUF:
        assert M == B * hw[0] * hw[1]
    return dict(kind=kind, tname=tname, K=K, N=N, ldo=N if out_f32 else ldo, mode=mode, prec=prec, out_prec=F32 if out_f32 else prec, out_f32=out_f32,
                index=index, rows_a=rows_a, B=B, M=M, a=a, a_dev=a_dev, named=named, w=w, b=b, r1=r1, r1_beyond=r1_beyond, res_mod=res_mod, f=f, hw=hw,
                coff=coff, rows_out=M * (f * f if kind == PIXSHUF else 1))


MUTANTS = {  # mutant -> is it something else than the identity on case c with M-tiles of BM rows?
    "index_ignored": lambda c, BM: True,
    "index_plus_one": lambda c, BM: True,
    "batch0": lambda c, BM: c["B"] > 1,
    "tail_clamped": lambda c, BM: c["M"] % BM > 1,
    "halo_other_tile": lambda c, BM: c["tname"] == "merge",
    "slice_coff_zero": lambda c, BM: c["kind"] == PIXSHUF and c["coff"] > 0,
    "res_row_m": lambda c, BM: c["kind"] == ROWS_RES and 0 < c["res_mod"] < c["M"],
    "wrap_lost": lambda c, BM: c["mode"][1] == "w32",
}


def MUTANT_ACTIVE(mut, c, BM=256):
    return MUTANTS[mut](c, BM)


def rows_read(c, mut, BM):
    idx, M = c["index"].clone(), c["M"]
    if mut == "index_ignored":
        idx = torch.arange(M)
    elif mut == "index_plus_one":
        idx = idx + 1
    elif mut == "batch0":
        idx = idx.reshape(c["B"], -1)[:1].expand(c["B"], -1).reshape(-1)
    elif mut == "tail_clamped" and M % BM:
        idx[M // BM * BM:] = idx[M - 1]
    elif mut == "halo_other_tile" and c["tname"] == "merge":
        idx = merge_table_py(2, 6, 3, 1, 40, halo_other=True)
    return idx


def product(A, Wt, c, dtype, mut):
    """A [M, K] . Wt [K, n]: fp64 at once, else summed k-tile by k-tile (32 elements for f32 operands, else 64) in `dtype`."""
    if dtype == torch.float64:
        return A.double() @ Wt.double()
    ke = 32 if c["prec"] == F32 else 64
    acc = torch.zeros(A.shape[0], Wt.shape[1], dtype=dtype)
    for k0 in range(0, c["K"], ke):
        acc += A[:, k0:k0 + ke].to(dtype) @ Wt[k0:k0 + ke].to(dtype)
    if mut == "wrap_lost" and c["mode"][1] == "w32":   # hi x W_lo becomes lo x W_lo
        hi, wl = R.f16_round(A), Wt - R.f16_round(Wt)
        acc += (A - hi).to(dtype) @ wl.to(dtype) - hi.to(dtype) @ wl.to(dtype)
    return acc


def evaluate(c, dtype=torch.float64, mut=None, BM=256):
    """-> (out [rows_out + TAIL, ldo] with the canary where the launch writes nothing, the written mask, pre = acc + bias over the written
    elements, the derived extra term over them or None). mut needs dtype fp32."""
    kind, M, N, ldo = c["kind"], c["M"], c["N"], c["ldo"]
    A = c["a"][rows_read(c, mut, BM)]
    out = canary(c["rows_out"] + TAIL, ldo).to(dtype)
    wrote = torch.zeros(out.shape, dtype=torch.bool)
    bias = c["b"].to(dtype) if c["b"] is not None else 0.0
    extra = None
    if kind == PIXSHUF:
        B, (h, w_), f = c["B"], c["hw"], c["f"]
        col = 0 if mut == "slice_coff_zero" else c["coff"]
        o4, w4 = out[:c["rows_out"]].view(B, f * h, f * w_, ldo), wrote[:c["rows_out"]].view(B, f * h, f * w_, ldo)
        if dtype == torch.float64 and mut is None:   # the definition: ConvTranspose2d k = s = f of the gathered map
            x = A.reshape(B, h, w_, c["K"]).permute(0, 3, 1, 2).double()
            o4[..., col:col + N] = F.conv_transpose2d(x, c["w"].double(), c["b"].double(), stride=f).permute(0, 2, 3, 1)
        else:
            for t in range(f * f):
                ky, kx = divmod(t, f)
                o4[:, ky::f, kx::f, col:col + N] = (product(A, c["w"][:, :, ky, kx], c, dtype, mut) + bias).reshape(B, h, w_, N)
        w4[..., col:col + N] = True
        return out, wrote, out[wrote], extra
    pre = product(A, c["w"].t(), c, dtype, mut) + bias
    v = pre
    if kind == ROWS_RES:
        m = torch.arange(M)
        v = pre + (c["r1_beyond"][m] if mut == "res_row_m" else c["r1"][m % c["res_mod"]])[:, :N].to(dtype)
        extra = (U * v.abs().double()).reshape(-1)
    out[:M, :N] = v
    wrote[:M, :N] = True
    return out, wrote, pre.reshape(-1), extra


def is_bad(got, c, ref, wrote, pre, extra):
    """What the GPU tests assert, as a predicate: finite, the canary where nothing is written, every written element inside its bound."""
    if not torch.isfinite(got).all() or not torch.equal(got[~wrote].float(), canary(*got.shape)[~wrote]):
        return True
    a32 = A_MFMA * pre.abs().max().item() / ref[wrote].abs().max().item()
    return rejects(got[wrote], ref[wrote], c["out_prec"], a32, extra)


def check(got, c, what):
    ref, wrote, pre, extra = evaluate(c)
    assert torch.isfinite(got).all(), what + ": non-finite values (a poisoned row was read)"
    can = canary(*got.shape)
    assert torch.equal(got[c["rows_out"]:], can[c["rows_out"]:]), what + ": rows behind M"
    assert torch.equal(got[~wrote], can[~wrote]), what + ": pad columns / channels outside the slice"
    a32 = A_MFMA * pre.abs().max().item() / ref[wrote].abs().max().item()
    return assert_close_in(got[wrote], ref[wrote], c["out_prec"], a32, extra=extra, what=what)


# (kind, table, N, ldo, kwargs): every (N, output) form of the GPU tests
ROWS_FORMS = [(264, 320, dict(bias=False)), (132, 192, dict(bias=False)), (128, 128, dict(out_f32=True)), (32, 32, dict(out_f32=True))]
RES_FORM = (48, 64, dict(res_mod=63))
# (table, h, w, f, Cout, coff): ldo = 2 round_up(Cout, 64) = 128
PS_FORMS = [("img36", 6, 6, 2, 64, 64), ("img36", 6, 6, 2, 36, 64), ("token", 7, 9, 2, 64, 64), ("token", 7, 9, 2, 36, 64), ("img36", 6, 6, 2, 64, 0),
            ("token", 7, 9, 4, 64, 64)]
KS = (128, 192)


def all_cases(mode):
    for K in KS:
        for tname in ("merge", "token", "random"):
            for N, ldo, kw in ROWS_FORMS:
                yield case(ROWS, tname, K, N, ldo, mode, **kw)
        yield case(ROWS_RES, "token", K, RES_FORM[0], RES_FORM[1], mode, **RES_FORM[2])
        for tname, h, w_, f, Cout, coff in PS_FORMS:
            yield case(PIXSHUF, tname, K, Cout, 128, mode, f=f, hw=(h, w_), coff=coff)


def what_of(c):
    return "kind%d %s K%d N%d ldo%d f%d coff%d f32out=%d %s" % (c["kind"], c["tname"], c["K"], c["N"], c["ldo"], c["f"], c["coff"], c["out_f32"], MODE_ID(c["mode"]))


@pytest.mark.parametrize("mode", MODES, ids=MODE_ID)
def test_checker_accepts_fp32_evaluation(mode):
    """Every case of the GPU tests: the fp32 evaluation of the reference formula, rounded once to the output type, passes the GPU tests' bound
    with under 1 % of the elements on the tie slack."""
    for c in all_cases(mode):
        ref, wrote, pre, extra = evaluate(c)
        got = ROUND[c["out_prec"]](evaluate(c, torch.float32)[0])
        assert not is_bad(got, c, ref, wrote, pre, extra), what_of(c)
        assert check(got, c, "fp32 evaluation, " + what_of(c))["slack_share"] < 0.01
        n = c["N"] * c["rows_out"]
        assert wrote.sum() == n and (wrote.shape[1] == c["ldo"])


@pytest.mark.parametrize("mode", MODES, ids=MODE_ID)
def test_checker_rejects_mutants(mode):
    """K = 192 (an odd k-tile count at 2-byte types); one (N, output) form per table for ROWS, every ROWS_RES and PIXSHUF form; tail_clamped at
    the M-tile of every tile size."""
    cases = [case(ROWS, "merge", 192, 264, 320, mode, bias=False), case(ROWS, "token", 192, 128, 128, mode, out_f32=True),
             case(ROWS, "random", 192, 132, 192, mode, bias=False), case(ROWS_RES, "token", 192, RES_FORM[0], RES_FORM[1], mode, **RES_FORM[2])]
    cases += [case(PIXSHUF, t, 192, Cout, 128, mode, f=f, hw=(h, w_), coff=coff) for t, h, w_, f, Cout, coff in PS_FORMS]
    for c in cases:
        ref, wrote, pre, extra = evaluate(c)
        for mut in MUTANTS:
            for BM in ((64, 128, 256) if mut == "tail_clamped" else (256,)):
                bad = ROUND[c["out_prec"]](evaluate(c, torch.float32, mut, BM)[0])
                assert is_bad(bad, c, ref, wrote, pre, extra) == MUTANT_ACTIVE(mut, c, BM), (mut, BM, what_of(c))
                if mut == "tail_clamped":
                    assert MUTANT_ACTIVE(mut, c, BM), "every M here leaves a partial last tile at every tile size"


# ---------------------------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    from burn_depth_amd.depth_pro import Device
    return Device(0)


def bits(t):
    return t.contiguous().view(torch.int32)


def launch(dev, c, tile, dense=False):
    """One call of the entry on canary-filled caller buffers -> (out on the CPU, the launch record). dense: index = NULL over a[index] gathered
    on the host. Asserts that a, index, w, res1 came back as they went."""
    o = ops()
    kind = c["kind"]
    a = (c["a"][c["index"]] if dense else c["a_dev"]).cuda()
    index = None if dense else c["index"].int().cuda()
    w, b = c["w"].cuda(), (c["b"].cuda() if c["b"] is not None else None)
    r1 = c["r1"].cuda() if c["r1"] is not None else None
    keep = [(t, t.clone()) for t in (a, index, w, r1) if t is not None]
    out = canary(c["rows_out"] + TAIL, c["ldo"]).cuda()
    kw = dict(B=c["B"], ph=c["hw"][0], pw=c["hw"][1], ps_f=c["f"], ps_coff=c["coff"]) if kind == PIXSHUF else {}
    o.indexed_gemm(dev, kind, a, index, w, b, c["prec"], tile, out=out, ldo=c["ldo"], out_f32=c["out_f32"], res1=r1, res_mod=c["res_mod"], **kw)
    for t, t0 in keep:
        assert torch.equal(bits(t) if t.dtype == torch.float32 else t, bits(t0) if t0.dtype == torch.float32 else t0), "an input of the launch changed"
    return out.cpu(), o.gemm_last_form()


def assert_form(f, c, tile):
    """The tile and, on the 256 x 256 tile, the kernel form the case was meant to reach (module docstring; gemm.hip gemm256_form)."""
    prec, N, ldo, kind = c["prec"], c["N"], c["ldo"], c["kind"]
    two_byte, split = prec != F32, prec == F16X2
    n_gemm = N * (c["f"] ** 2 if kind == PIXSHUF else 1)
    want = tile if tile != TAUTO else lib().md_gemm_pick_tile(c["M"], n_gemm, c["K"] * terms_of(c["mode"]), prec)
    assert f["tile"] == want, (f, want)
    if tile == TAUTO and n_gemm <= 32:
        assert f["tile"] == T256x32
    fast = kind == PIXSHUF and two_byte and N % 8 == 0 and ldo % 8 == 0 and c["coff"] % 8 == 0
    assert f["ps_fast"] == int(fast), f
    if f["tile"] != T256:
        assert f["family"] == -1, f
        return
    if kind == PIXSHUF:
        ek = EK_GENERIC if (split and not fast) else EK_PIXSHUF
    elif kind == ROWS_RES:
        ek = EK_GENERIC
    else:
        ek = EK_STORE if (two_byte and N % 8 == 0 and ldo % 8 == 0 and not (split and c["out_f32"])) else EK_GENERIC
    assert (f["family"], f["ek"], f["fold"], f["qkv"], f["conv"], f["diag"]) == (0, ek, 0, 0, 0, 0), (f, ek)
    assert f["blocks"] == f["grid"] == -(-c["M"] // 256) * -(-n_gemm // 256), f


def run_case(dev, c):
    for tile in TILES:
        what = what_of(c) + " tile%d" % tile
        got, f = launch(dev, c, tile)
        assert_form(f, c, tile)
        check(got, c, what)
        dense, fd = launch(dev, c, tile, dense=True)
        assert fd == f, (what, f, fd)
        assert torch.equal(bits(got), bits(dense)), what + ": the gathered launch and the dense launch over a[index] differ"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_ID)
@pytest.mark.parametrize("tname", ["merge", "token", "random"])
def test_gathered_rows_against_fp64(dev, tname, mode):
    """gemm_rows with a table: enc_proj (T out, no bias; the 16-byte store kinds at N = 264 / 320, the generic epilogue at N = 132) and
    fov_proj (bias, fp32 rows; N = 32 is TILE_AUTO's 256 x 32 tile), K = 128 | 192, every tile; poisoned rows, the dense twin, the canary."""
    for K in KS:
        for N, ldo, kw in ROWS_FORMS:
            run_case(dev, case(ROWS, tname, K, N, ldo, mode, **kw))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_ID)
def test_stage_projection_with_residual_table_against_fp64(dev, mode):
    """The Depth-Anything-v3 stage projection: the token table of B = 2 images, a bias and res1[m % 63]."""
    for K in KS:
        run_case(dev, case(ROWS_RES, "token", K, RES_FORM[0], RES_FORM[1], mode, **RES_FORM[2]))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_ID)
@pytest.mark.parametrize("form", PS_FORMS, ids=lambda s: "%s_%dx%d_f%d_C%d_coff%d" % s)
def test_gathered_pixel_shuffle_against_fp64(dev, form, mode):
    """deconv2 with a table: the low-resolution deconvolution into channels [coff, coff + Cout) of pixels of 128."""
    tname, h, w_, f, Cout, coff = form
    for K in KS:
        run_case(dev, case(PIXSHUF, tname, K, Cout, 128, mode, f=f, hw=(h, w_), coff=coff))


@pytest.mark.gpu
def test_refusals_launch_nothing(dev):
    """Null arguments, K off the k-tile, N % 4, a row too narrow for the slice, fp8, an index outside a: each is the entry's own error and the
    output keeps the canary (nothing was launched)."""
    from burn_depth_amd import _lib
    o = ops()
    c = case(ROWS, "random", 128, 32, 32, MODES[0], out_f32=True)
    a, index, w, b = c["a_dev"].cuda(), c["index"].int().cuda(), c["w"].cuda(), c["b"].cuda()
    out = canary(c["M"] + TAIL, 32).cuda()

    def refused(code, **kw):
        args = dict(kind=ROWS, a=a, index=index, w=w, bias=b, precision=c["prec"], out=out, ldo=32, out_f32=True)
        args.update(kw)
        with pytest.raises(_lib.MdError) as e:
            o.indexed_gemm(dev, args.pop("kind"), args.pop("a"), args.pop("index"), args.pop("w"), args.pop("bias"), args.pop("precision"), **args)
        assert e.value.code == code and "indexed_gemm" in str(e.value), str(e.value)
        assert torch.equal(out.cpu(), canary(c["M"] + TAIL, 32)), "a refused call wrote"

    for bad_index in (index.clone().index_fill_(0, torch.tensor([299]).cuda(), 97), index.clone().index_fill_(0, torch.tensor([0]).cuda(), -1)):
        refused(_lib.MD_ERR_INVALID_ARG, index=bad_index)
    refused(_lib.MD_ERR_INVALID_ARG, precision=FP8)
    refused(_lib.MD_ERR_UNSUPPORTED, a=torch.zeros(97, 96).cuda(), w=torch.zeros(32, 96).cuda())              # bf16: k-tiles of 64
    refused(_lib.MD_ERR_UNSUPPORTED, w=torch.zeros(30, 128).cuda(), bias=torch.zeros(30).cuda())               # N % 4
    wide = canary(c["M"] + TAIL, 40).cuda()
    refused(_lib.MD_ERR_SHAPE, w=torch.zeros(48, 128).cuda(), bias=torch.zeros(48).cuda(), out=wide, ldo=40)   # 48 channels in rows of 40
    cp = case(PIXSHUF, "img36", 128, 64, 128, MODES[0], f=2, hw=(6, 6), coff=64)
    ps = dict(kind=PIXSHUF, a=cp["a_dev"].cuda(), index=cp["index"].int().cuda(), w=cp["w"].cuda(), bias=cp["b"].cuda(), out_f32=False, B=2, ph=6, pw=6, ps_f=2)
    refused(_lib.MD_ERR_SHAPE, out=canary(cp["rows_out"], 120).cuda(), ldo=120, ps_coff=64, **ps)              # the slice [64, 128) in pixels of 120
    refused(_lib.MD_ERR_INVALID_ARG, out=canary(cp["rows_out"], 128).cuda(), ldo=128, ps_coff=64, **dict(ps, bias=None))
    d = _lib.MdIndexedGemm()
    assert lib().md_op_indexed_gemm(dev.handle, C.byref(d), None) == _lib.MD_ERR_INVALID_ARG                    # null a / w / out
    assert lib().md_op_indexed_gemm(dev.handle, None, None) == _lib.MD_ERR_INVALID_ARG
