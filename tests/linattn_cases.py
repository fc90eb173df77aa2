"""Cases and operands of the per-launch linear-attention tests (tests/test_gpu_linattn_kernels.py, tests/test_linattn_reference_cpu.py).
The shapes are the smallest at which each mechanism can fail - empty waves and slots, ragged last sub-tiles, a one-pixel last block, the
sub-tile counts the batch rule reaches, every merge_fold path - none is a workload shape.  Operands sit on the grids
tests/linattn_reference.py derives its bounds for."""
import torch

from tests import linattn_reference as R

PRECS = ("bf16", "fp16", "fp16x2")
CS = (64, 128)
KNOBS = ("DEX_OUT2_MIN",)
G = 0.75                                         # the Rezero gate

# (npix, nsub, B): nblk = ceil(npix / (128 nsub))
CTX_SHAPES = ((1, 1, 1), (33, 1, 1), (129, 1, 1), (300, 2, 1), (1000, 3, 1), (1100, 4, 1), (1030, 8, 1), (200, 1, 3))
CTX_FORMS = ((False, False), (True, False), (True, True))          # (headwaves, rows)
MERGE_NBLK = (1, 7, 8, 9, 64, 65, 128, 129, 192, 193, 320)
TAIL_NPIX = (1, 33, 127, 129, 200)
TAIL_B = (1, 3)
PRO_H, PRO_W, PRO_B = 40, 5, 2
PRO_FLS = (0, 14, 1, 3, 5, 7, 9, 11, 13, 15)     # bit 0 h2 16-bit, 1 res 16-bit, 2 Xout 16-bit, 3 res under the mask; even: the run-time-flag form
FP32_N = (300, 700, 4200)                        # nchunks 1, 2, 9 of 512; none a multiple of the chunk
CHAIN = dict(npix=300, nsub=2, B=2)


def nblk_of(npix, nsub):
    return (npix + 128 * nsub - 1) // (128 * nsub)


def hw_supported(C, prec):
    return not (prec == "fp16x2" and C == 128)


def kvctx_form(C, headwaves, rows, pro=False, fl=-1):
    flt = fl if (pro and fl % 2 == 1) else -1
    base = f"linattn_kvctx_hw_kernel C={C}" if headwaves else f"linattn_kvctx_kernel C={C}"
    return f"{base} PRO={int(pro)} FL={flt}" + (f" ROWS={int(rows)}" if headwaves else "")


def tail_form(C, kind):
    return {"direct": f"linattn_out2_direct_kernel C={C}", "hw0": f"linattn_out2_hw_kernel C={C} rows=0",
            "hw1": f"linattn_out2_hw_kernel C={C} rows=1", "throughput": f"linattn_out2_kernel C={C} (throughput)"}[kind]


def merge_form(nblk):
    per = (nblk + 7) // 8
    return f"linattn_merge_kernel merge_fold<{8 if per <= 8 else 16 if per <= 16 else 24}>"


def expected_forms(prec):
    """Every instantiation the launchers' switch statements can take in the mode's build."""
    out = set()
    for C in CS:
        for hw, rows in CTX_FORMS:
            if hw and not hw_supported(C, prec):
                continue
            out.add(kvctx_form(C, hw, rows))
            for fl in PRO_FLS:
                out.add(kvctx_form(C, hw, rows, True, fl))
        out |= {tail_form(C, k) for k in ("direct", "hw0", "hw1", "throughput")}
    return out | {merge_form(n) for n in MERGE_NBLK}


# stress rows of Wkv: (head, channel) of k, and one v row
K_RAMP, K_SPIKE, K_CONST, K_LOW, V_ZERO = (0, 0), (1, 1), (2, 2), (3, 3), (1, 0)


def make_weights(C, prec, seed=0):
    """Wqkv [384, C], Wout [C, 128], bout [C] fp32.  Wqkv on the grids of the reference's docstring; the k-stress rows hold +-1/2."""
    g = torch.Generator().manual_seed(7919 * C + seed)
    mag = torch.randint(8, 16, (384, C), generator=g).double() / 64
    sign = torch.randint(0, 2, (384, C), generator=g).double() * 2 - 1
    W = mag * sign
    lo = torch.randint(1, 4, (384, C), generator=g).double() * (torch.randint(0, 2, (384, C), generator=g).double() * 2 - 1) * R.LO_GRID
    if prec == "fp16x2":
        W = W + lo
    q4 = C // 4
    kr = lambda hd: 128 + 32 * hd[0] + hd[1]
    W[kr(K_RAMP)] = 0
    W[kr(K_RAMP), :q4] = 0.5
    W[kr(K_SPIKE)] = 0
    W[kr(K_SPIKE), q4:2 * q4] = 0.5
    W[kr(K_CONST)] = 0
    W[kr(K_LOW), :3 * q4] = 0
    W[kr(K_LOW), 2 * q4:3 * q4] = -0.5
    W[256 + 32 * V_ZERO[0] + V_ZERO[1], q4:] = 0
    Wout = torch.randn(C, 128, generator=g) * 0.1
    bout = torch.randn(C, generator=g) * 0.5
    return W.float(), Wout, bout


def spike_pixels(npix):
    return sorted({min(5, npix - 1), npix - 1})


def make_x(C, B, npix, seed=0):
    """x [B, npix, C] fp32 = x^ (1 +- 2^-13), x^ on the 2^-3 grid in [-1, 1].  Channel quarters: a thermometer ramp (the maximum of the
    k ramp row moves with every few pixels; descending for odd b), -1 with +1 spikes early and in the last pixel, the constant 1, random."""
    g = torch.Generator().manual_seed(104729 * C + 31 * npix + B + seed)
    q4 = C // 4
    xh = torch.randint(-8, 9, (B, npix, C), generator=g).double() / 8
    T = torch.arange(npix) * (16 * q4) // npix
    ramp = -1 + (T[:, None] - 16 * torch.arange(q4)[None, :]).clamp(0, 16).double() / 8
    for b in range(B):
        xh[b, :, :q4] = ramp if b % 2 == 0 else ramp.flip(0)
    xh[:, :, q4:2 * q4] = -1
    for s in spike_pixels(npix):
        xh[:, s, q4:2 * q4] = 1
        xh[:, s, :q4] = 0
    xh[:, :, 2 * q4:3 * q4] = 1
    eps = (torch.randint(0, 2, xh.shape, generator=g).double() * 2 - 1) * 2.0 ** -13
    return (xh * (1 + eps)).float()


def make_pro(C, prec, fl, with_res, seed=0):
    """Inputs of a PRO launch at H = 40, W = 5, B = 2: h2 and res as the flags store them (16-bit VALUES as fp32 where they are 16-bit),
    GroupNorm statistics of h2, gamma, beta, a mask [B, 2 W] with zeros inside every sub-tile (column w at mask[b, w * mask_ws])."""
    g = torch.Generator().manual_seed(15485863 + 100 * C + fl + (50 if with_res else 0) + seed)
    B, N = PRO_B, PRO_H * PRO_W
    h2 = torch.randn(B, N, C, generator=g) * 1.5 + 0.25
    res = torch.randn(B, N, C, generator=g) if with_res else None
    lp = R.LP_DTYPE[prec]
    if fl & 1:
        h2 = h2.to(lp).float()
    if with_res and fl & 2:
        res = res.to(lp).float()
    gamma = 1 + 0.25 * torch.randn(C, generator=g)
    beta = 0.25 * torch.randn(C, generator=g)
    hg = h2.double().reshape(B, N, 8, C // 8).permute(0, 2, 1, 3).reshape(B, 8, -1)
    mean, meansq = hg.mean(-1), (hg * hg).mean(-1)
    cols = torch.ones(B, PRO_W)
    cols[0, 3] = 0
    cols[1, 0] = 0
    cols[1, 4] = 0
    return dict(h2=h2, res=res, gamma=gamma, beta=beta, mean=mean, meansq=meansq, cols=cols)


def mask_of(cols, mask_ws):
    """[B, W * mask_ws] with column w at [b, w * mask_ws]; the words between hold a value the kernels must not read."""
    B, W = cols.shape
    m = torch.full((B, W * mask_ws), 7.0)
    m[:, ::mask_ws] = cols
    return m


def make_partials(nblk, B, seed=0):
    """Synthetic partials for the merge kernel: m spread over +-40, one -inf partial among finite ones (where there are three or more),
    s in [1, 100], c normal."""
    g = torch.Generator().manual_seed(2750159 + 17 * nblk + B + seed)
    pm = (torch.rand(B, 4, nblk, 32, generator=g) * 80 - 40).float()
    ps = (torch.rand(B, 4, nblk, 32, generator=g) * 99 + 1).float()
    pc = torch.randn(B, 4, nblk, 32, 32, generator=g)
    if nblk >= 3:
        pm[:, :, nblk // 2, ::3] = -float("inf")
    return pm, ps, pc


def make_w2(C, B, prec, seed=0):
    """A synthetic W2 for the tail alone: 16-bit VALUES of magnitude about 2^-6."""
    g = torch.Generator().manual_seed(32452843 + C + B + seed)
    return (torch.randn(B, C, 128, generator=g) * 2.0 ** -6).to(R.LP_DTYPE[prec]).float()


def make_qkv(n, B, seed=0):
    """fp32-mode operands: qkv [B, n, 384], k with a wide range."""
    g = torch.Generator().manual_seed(49979687 + n + B + seed)
    qkv = torch.randn(B, n, 384, generator=g)
    qkv[..., 128:256] *= 4
    return qkv
