"""bpm_kv_source_fwd / _bwd (key / value sources embedded and normalised in one pass) on the GPU.

Kernel level: against the launches they replace (embed_pos_fwd -> ln_fwd, ln_bwd -> embed_pos_bwd) on the same inputs,
bit for bit, and against an fp64 torch reference at the tolerances tests/test_rowops_gpu.py uses for those kernels; every
output is a view into a guarded buffer.  Three problems of different sizes per launch ((5, 3), (37, 7) and 1037 x 1 rows:
pick() and the row loops iterate, and the odd count leaves one wave of the backward with a live and a dead row), widths
24 / 300 / 768 / 1024 (1 .. 4 chunks per lane; 300: ragged last chunk set and pad columns up to ld = 320), xk is xv and
xk distinct from xv, pad positions, all-zero rows, positions other than 0 / 1, dropout 0.25 and 0, both compute types,
separate and merged gradients.

Engine level: one small crossmodal plan run with BPMULT_KV_FUSED=1 and =0."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from bpmult_amd import _lib, engine, ops  # noqa: E402
from bpmult_amd.ops import BPM_BF16, BPM_F32, pad32  # noqa: E402
from test_kernels_gpu import DEV, DT, close, drop_mult, rnd  # noqa: E402
from test_rowops_gpu import Guarded, bits, ct_out, ln_ref64  # noqa: E402

PROBS = [(5, 3, 0, 1), (37, 7, 3, 2), (1037, 1, 0, 1)]          # (S, B, pos0, pos_stride)
SITE_K, SITE_V, SEED = 11, 12, 4321
TABLE_ROWS = 1037 + 3


def _source(j, S, B, d, seed):
    x = rnd(S, B, d, seed=seed + j)
    x[1 + j, 0, 0] = 0.0                          # pad position: channel 0 is zero, the other channels are not
    x[-(1 + j):] = 0.0                            # all-zero rows: variance 0, rstd = 1 / sqrt(eps)
    return x


@functools.lru_cache(maxsize=4)
def case(d):
    """Host inputs of the three problems (shared by both compute types)."""
    xk = [_source(j, S, B, d, 100) for j, (S, B, _, _) in enumerate(PROBS)]
    xv = [_source(j + 1, S, B, d, 200) for j, (S, B, _, _) in enumerate(PROBS)]
    gk = [rnd(S * B, d, seed=300 + j) for j, (S, B, _, _) in enumerate(PROBS)]
    gv = [rnd(S * B, d, seed=400 + j) for j, (S, B, _, _) in enumerate(PROBS)]
    return xk, xv, gk, gv


@functools.lru_cache(maxsize=32)
def reference(d, j, p, src, side):
    """fp64: normalised embedded source, its statistics and the source gradient of problem j; src 0: xk, 1: xv."""
    xk, xv, gk, gv = case(d)
    S, B, pos0, stride = PROBS[j]
    x, g = (xv if src else xk)[j], (gv if side else gk)[j]
    table = engine.sinusoid_table(TABLE_ROWS, d, torch.device(DEV)).cpu()
    mult = drop_mult((S, B, d), p, SEED, SITE_V if side else SITE_K).double().view(S * B, d)
    pos = torch.where(x[:, :, 0] != 0, pos0 + stride * torch.arange(S)[:, None] + 1, torch.zeros(1, dtype=torch.long))
    scale = math.sqrt(d)
    e = (scale * x.double() + table.double()[pos]).view(S * B, d) * mult
    y, dx, mean, rstd, _ = ln_ref64(e, torch.ones(d), None, g)
    plain = (x.view(S * B, d) != 0).any(1)
    return y, mean, rstd, scale * mult * dx, plain


def old_route(d, dtype, p, same):
    """embed_pos_fwd -> ln_fwd (gamma 1, beta 0) and ln_bwd -> embed_pos_bwd: khat, vhat, four statistics, dxk, dxv per problem."""
    xk, xv, gk, gv = case(d)
    ld, scale = pad32(d), math.sqrt(d)
    table = engine.sinusoid_table(TABLE_ROWS, d, torch.device(DEV))
    ones, zeros = torch.ones(d, device=DEV), torch.zeros(d, device=DEV)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device=DEV, dtype=dt)
    emb, fwd, bwd, emb_b, res, keep = [], [], [], [], [], []
    for j, (S, B, pos0, stride) in enumerate(PROBS):
        R = S * B
        srck = xk[j].to(DEV)
        srcv = srck if same else xv[j].to(DEV)
        r = dict(khat=z(R, ld, dt=ops.ct_torch(dtype)), vhat=z(R, ld, dt=ops.ct_torch(dtype)), mk=z(R), rk=z(R), mv=z(R), rv=z(R),
                 dxk=z(S, B, d), dxv=z(S, B, d))
        ke, ve, dke, dve, gkd, gvd = z(R, d), z(R, d), z(R, d), z(R, d), gk[j].to(DEV), gv[j].to(DEV)
        keep += [srck, srcv, ke, ve, dke, dve, gkd, gvd]          # the problem structs hold raw pointers only
        emb += [ops.embed_problem(srck, ke, S, B, drop_p=p, drop_site=SITE_K, pos0=pos0, pos_stride=stride),
                ops.embed_problem(srcv, ve, S, B, drop_p=p, drop_site=SITE_V, pos0=pos0, pos_stride=stride)]
        fwd += [ops.ln_problem(ke, ones, zeros, r["mk"], r["rk"], R, out=r["khat"], ldo=ld),
                ops.ln_problem(ve, ones, zeros, r["mv"], r["rv"], R, out=r["vhat"], ldo=ld)]
        bwd += [ops.ln_problem(ke, ones, None, r["mk"], r["rk"], R, dy=gkd, ldy=d, dx=dke),
                ops.ln_problem(ve, ones, None, r["mv"], r["rv"], R, dy=gvd, ldy=d, dx=dve)]
        emb_b += [ops.embed_problem(dke, r["dxk"], S, B, drop_p=p, drop_site=SITE_K),
                  ops.embed_problem(dve, r["dxv"], S, B, drop_p=p, drop_site=SITE_V)]
        res.append(r)
    ops.embed_pos_fwd(emb, table, d, scale, SEED)
    ops.ln_fwd(dtype, fwd, d)
    ops.ln_bwd(bwd, d, dtype, SEED)
    ops.embed_pos_bwd(emb_b, d, scale, SEED)
    torch.cuda.synchronize()
    return res


def fused_route(d, dtype, p, same):
    xk, xv, gk, gv = case(d)
    ld, scale = pad32(d), math.sqrt(d)
    table = engine.sinusoid_table(TABLE_ROWS, d, torch.device(DEV))
    probs, merged, res, keep = [], [], [], []
    for j, (S, B, pos0, stride) in enumerate(PROBS):
        R = S * B
        srck = xk[j].to(DEV)
        srcv = srck if same else xv[j].to(DEV)
        gkd, gvd = gk[j].to(DEV), gv[j].to(DEV)
        keep += [srck, srcv, gkd, gvd]
        r = dict(khat=ct_out(R, ld, dtype=dtype), vhat=ct_out(R, ld, dtype=dtype), mk=Guarded(R), rk=Guarded(R), mv=Guarded(R),
                 rv=Guarded(R), dxk=Guarded(S, B, d), dxv=Guarded(S, B, d), dx=Guarded(S, B, d))
        kw = dict(khat=r["khat"].v, vhat=r["vhat"].v, ld=ld, stats_k=(r["mk"].v, r["rk"].v), stats_v=(r["mv"].v, r["rv"].v),
                  gk=gkd, gv=gvd, drop_p=p, drop_site_k=SITE_K, drop_site_v=SITE_V, pos0=pos0, pos_stride=stride)
        probs.append(ops.kv_source_problem(srck, srcv, S, B, dxk=r["dxk"].v, dxv=r["dxv"].v, **kw))
        merged.append(ops.kv_source_problem(srck, srcv, S, B, dxk=r["dx"].v, dxv=None, **kw))
        res.append(r)
    ops.kv_source_fwd(dtype, probs, table, d, scale, SEED)
    ops.kv_source_bwd(probs, table, d, scale, SEED)
    ops.kv_source_bwd(merged, table, d, scale, SEED)
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("d,dtype", [(d, dt) for d in (24, 300, 768, 1024) for dt in DT])
def test_fused_against_two_kernel_route_and_fp64(d, dtype):
    ld = pad32(d)
    tf = 2e-5 if dtype == BPM_F32 else 1e-2
    for p in (0.25, 0.0):
        for same in (True, False):
            old, new = old_route(d, dtype, p, same), fused_route(d, dtype, p, same)
            for j, (o, n) in enumerate(zip(old, new)):
                what = f"d={d} p={p} same={same} problem {j}: "
                for k, g in n.items():
                    g.check(what + k)
                diff = {k: int((bits(o[k]) != bits(n[k].v)).sum()) for k in ("khat", "vhat", "mk", "rk", "mv", "rv", "dxk", "dxv")}
                diff["merged"] = int((bits(n["dx"].v) != bits(o["dxk"] + o["dxv"])).sum())
                assert not any(diff.values()), what + f"elements that differ from the two-kernel route (merged: from dxk + dxv): {diff}"
                for side, (hat, m, r, dx) in enumerate((("khat", "mk", "rk", "dxk"), ("vhat", "mv", "rv", "dxv"))):
                    y, mean, rstd, dxr, plain = reference(d, j, p, 0 if same or side == 0 else 1, side)
                    close(n[hat].v[:, :d].float(), y, tf, what + hat)
                    assert (n[hat].v[:, d:].float() == 0).all(), what + hat + " pad columns"
                    close(n[m].v, mean, 2e-5, what + m)
                    close(n[r].v, rstd, 2e-5, what + r)
                    got = n[dx].v.view(-1, d)
                    close(got, dxr, 1e-4, what + dx)
                    # the all-zero rows have rstd = 316 and set the scale above: the ordinary rows on their own scale
                    close(got[plain.to(DEV)], dxr[plain], 1e-4, what + dx + ", ordinary rows")
                    assert (~plain).any() and ((rstd[~plain] - 1e-5 ** -0.5).abs() < 1e-9).all()     # variance 0: rstd = 1 / sqrt(eps)


def test_outside_the_domain_is_refused():
    import ctypes as C
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    S, B = 5, 3

    def rc(d, ld=None, skew=0, dtype=BPM_BF16, table_rows=TABLE_ROWS):
        ld = pad32(d) if ld is None else ld
        R = S * B
        x = Guarded(S, B, d, start=torch.ones(S, B, d), skew=skew)
        table = torch.zeros(TABLE_ROWS, d, device=DEV)
        khat, vhat = ct_out(R, max(ld, d), dtype=dtype), ct_out(R, max(ld, d), dtype=dtype)
        st = [Guarded(R) for _ in range(4)]
        g, dxk, dxv = torch.zeros(R, d, device=DEV), Guarded(S, B, d), Guarded(S, B, d)
        p = ops.kv_source_problem(x.v, x.v, S, B, khat=khat.v, vhat=vhat.v, ld=ld, stats_k=(st[0].v, st[1].v), stats_v=(st[2].v, st[3].v),
                                  gk=g, gv=g, dxk=dxk.v, dxv=dxv.v)
        r = (L.bpm_kv_source_fwd(dtype, C.byref(p), 1, table.data_ptr(), table_rows, d, 1.0, 1e-5, 0, s),
             L.bpm_kv_source_bwd(C.byref(p), 1, table.data_ptr(), table_rows, d, 1.0, 0, s))
        torch.cuda.synchronize()
        for t in [khat, vhat, dxk, dxv] + st:
            t.check(f"refused launch d={d}")
        return r

    assert rc(24) == (0, 0)
    assert rc(50) == (-1, -1)                               # d % 4 != 0
    assert rc(1028) == (-1, -1)                             # d > 1024
    assert rc(24, skew=1) == (-1, -1)                       # source 4 bytes off a 16-byte boundary
    assert rc(24, ld=20)[0] == -1 and rc(24, ld=30)[0] == -1
    assert rc(24, table_rows=S) == (-1, -1)                 # the last row's position lies outside the table
    with pytest.raises(RuntimeError):
        x = torch.ones(S, B, 50, device=DEV)
        ops.kv_source_bwd([ops.kv_source_problem(x, x, S, B, stats_k=(x, x), stats_v=(x, x), gk=x, gv=x, dxk=x)],
                          torch.zeros(8, 50, device=DEV), 50, 1.0)


def _plan_run(monkeypatch, fused, prec, merge):
    """A fresh two-encoder crossmodal plan (hidden 24, 2 layers, B = 2, T = 5, S = 7 / 8) with deterministic parameters:
    one training forward + backward; outputs, input gradients and parameter gradients as host tensors."""
    from bpmult_amd.models.encoder import TransformerEncoder
    monkeypatch.setenv("BPMULT_KV_FUSED", "1" if fused else "0")
    d, H, L, B, Tq = 24, 2, 2, 2, 5
    mods = [TransformerEncoder(d, H, L, attn_dropout=0.1, relu_dropout=0.1, res_dropout=0.1, embed_dropout=0.25, attn_mask=True).to(DEV)
            for _ in range(2)]
    with torch.no_grad():
        for j, m in enumerate(mods):
            for i, (k, q) in enumerate(m.named_parameters()):
                q.copy_((0.2 * rnd(*q.shape, seed=1000 * j + i) + (1.0 if "layer_norm" in k and k.endswith("weight") else 0.0)).to(DEV))
    st = engine.ParamStore([(f"e{j}.{k}", q) for j, m in enumerate(mods) for k, q in m.named_parameters()], prec)
    for j in range(2):
        engine.register_encoder_shadows(st, f"e{j}.", d, L)
    st.finalize_shadows()
    cfg = engine.GroupCfg(d, H, L, 0.1, 0.1, 0.25, True, False)
    plan = engine.EncoderGroupPlan(st, cfg, [engine.EncoderDesc(f"e{j}.", j, Tq, 7 + j, 0.1) for j in range(2)], B)
    assert plan._kv_fused == fused
    if merge:
        assert plan.merge_kv_grads()
    xq = [rnd(Tq, B, d, seed=50 + j).to(DEV) for j in range(2)]
    xk = [_source(j, 7 + j, B, d, 60).to(DEV) for j in range(2)]
    ws = [rnd(Tq, B, d, seed=70 + j).to(DEV) for j in range(2)]
    st.refresh_shadows()
    ys = [y.clone() for y in plan.forward(xq, xk, xk, seed=77, training=True)]
    st.begin_backward()
    gq, gk, gv = plan.backward(ws)
    torch.cuda.synchronize()
    grads = {n: st.g(n).clone().cpu() for n in st.params}
    cp = lambda ts: [None if t is None else t.clone().cpu() for t in ts]
    return cp(ys), cp(gq), cp(gk), cp(gv), grads


@pytest.mark.parametrize("prec", DT)
def test_plan_fused_and_two_kernel_route_agree(monkeypatch, prec):
    """The encoder outputs, the input gradients and the gradients of the weight matrices are the same bits with
    BPMULT_KV_FUSED=1 and =0; the merged key / value gradient is the fp32 sum of the two.  The remaining parameter
    gradients (biases, LayerNorm affines, the folded in_proj rows) are sums that several workgroups add to with float
    atomics, in an order that differs from run to run of ONE route: those are held to 1e-6 of their largest element."""
    ys0, gq0, gk0, gv0, g0 = _plan_run(monkeypatch, False, prec, False)
    ys1, gq1, gk1, gv1, g1 = _plan_run(monkeypatch, True, prec, False)
    ys2, gq2, gk2, gv2, g2 = _plan_run(monkeypatch, True, prec, True)
    for a, b, c in zip(ys0 + gq0, ys1 + gq1, ys2 + gq2):
        assert torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(c))
    for a, b in zip(gk0 + gv0, gk1 + gv1):
        assert torch.equal(bits(a), bits(b))
    assert gv2 == [None, None]
    for k0, v0, m in zip(gk0, gv0, gk2):
        assert torch.equal(bits(m), bits(k0 + v0))
    exact = ("fc1.weight", "fc2.weight", "out_proj.weight")
    assert set(g0) == set(g1) == set(g2) and any(n.endswith(exact) for n in g0)
    for n in g0:
        for g in (g1[n], g2[n]):
            if n.endswith(exact):
                assert torch.equal(bits(g0[n]), bits(g)), n
            else:
                close(g, g0[n], 1e-6, n)
