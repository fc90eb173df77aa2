"""ctypes loader of the test-only launch shim (tests/kshim/kshim.hip, built by dex_tts_amd/build.py next to the library).

The shim fills the library's parameter structs from flat descriptors and runs ONE launch.  This side mirrors the descriptors,
checks every tensor against the extent its descriptor implies BEFORE the call (the shim sees pointers only), and returns the kernel
instantiation the launcher picked.  A descriptor the shim rejects raises ShimError: a mistyped case is an error, never a launch."""
import ctypes as C
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libkshim.so")
PREC = {"bf16": 1, "fp16": 2, "fp16x2": 3}
LP_DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp16x2": torch.float16}
ERRORS = {-1: "precision", -2: "null pointer", -3: "shape", -4: "unsupported by the library's predicates", -5: "no such form",
          -6: "stride / offset"}
PREDICATES = {"conv3x3_bf16_supported": 0, "conv3x3_bf16_tail_supported": 1, "conv3x3_bf16_res_supported": 2,
              "conv3x3_bf16_xb_supported": 3, "conv3x3_plain_lp_in_supported": 4, "conv3x3_cat_lp_in_supported": 5,
              "conv3x3_res2_form": 6, "conv_down_supported": 7, "convt_up_supported": 8, "dit_rowchain_supported": 9,
              "dit_rowchain64_form": 10, "dit_rowchain_cluster_form": 11, "dit_rowchain_cluster_local_fits": 12,
              "dit_rowchain_cluster_xcds": 13}
DIT_CLUSTER = 4                                  # csrc/kernels.h
DIT_CLUSTER_SLAB_FLOATS = 2 * DIT_CLUSTER * (32 * 256 + 256)
DIT_CLUSTER_FLAG_WORDS = 2 * DIT_CLUSTER
GN_SLOTS = 32


class ShimError(RuntimeError):
    pass


def _ptrs(*names):
    return [(n, C.c_void_p) for n in names]


def _ints(*names):
    return [(n, C.c_int32) for n in names]


class KsConv3(C.Structure):
    _fields_ = (_ptrs("X", "Wbf", "Wfrag", "bias", "mask", "Y", "pro_stats", "pro_gamma", "pro_beta", "pro_tadd", "pro_res", "pro_xout",
                      "res2_w", "res2_b", "res2_mu", "res2_x", "res2_spk", "res2_scal", "res_w", "res_b", "res_wfrag", "res_y", "gn_stats")
                + [("mask_bstride", C.c_int64), ("w_lo_off", C.c_int64), ("res_lo_off", C.c_int64)]
                + _ints("precision", "H", "W", "Cin", "Cout", "B", "ldx", "x_coff", "mask_ws", "step", "row_bstride", "x_bf16", "y_bf16",
                        "xout_lp", "res2_scal_stride", "res2_planes"))


class KsConvDown(C.Structure):
    _fields_ = (_ptrs("X", "Wfrag", "bias", "inmask", "Y") + [("xb", C.c_int64), ("mask_bstride", C.c_int64)]
                + _ints("precision", "a_lp", "c_lp", "ldx", "x_coff", "H", "W", "ldy", "y_coff", "inmask_ws", "B", "C"))


class KsConvTUp(C.Structure):
    _fields_ = (_ptrs("X", "Wfrag0", "Wfrag1", "Wfrag2", "Wfrag3", "bias", "inmask", "Y") + [("xb", C.c_int64), ("mask_bstride", C.c_int64)]
                + _ints("precision", "a_lp", "c_lp", "ldx", "x_coff", "H", "W", "ldy", "y_coff", "inmask_ws", "B", "C"))


class KsAttn(C.Structure):
    _fields_ = (_ptrs("Qh", "Kh", "Vt", "O", "ml") + [("o_sstride", C.c_int64)]
                + _ints("N", "Npad", "B", "ksplit", "o_lp", "tail_g", "tail_ks", "half_g", "half_n", "precision"))


class KsRowChain(C.Structure):
    _fields_ = (_ptrs("X", "O", "ml", "Wp", "W1", "W2", "Wq", "bp", "b1", "b2", "bq", "ada", "next_shift", "next_scale", "Qh", "Kh", "Vt",
                      "Qin", "Kin", "Vin", "xslab", "xflag")
                + [("o_sstride", C.c_int64), ("next_step_stride", C.c_int64)]
                + _ints("precision", "B", "N", "Npad", "ksplit", "qkv_only", "attn_inline", "step", "row_bstride", "o_lp", "tail_row0",
                        "tail_ks", "xlocal")
                + [("epoch", C.c_uint32), ("qscale", C.c_float)])


class KsLinKvCtx(C.Structure):
    _fields_ = (_ptrs("X", "Wkv", "H2", "gn_stats", "gamma", "beta", "res", "mask", "part_m", "part_s", "part_c", "Xout")
                + [("xb", C.c_int64), ("resb", C.c_int64), ("mask_bstride", C.c_int64), ("wkv_lo_off", C.c_int64)]
                + _ints("precision", "npix", "C", "B", "ldx", "x_coff", "nsub", "nblk", "headwaves", "rows", "ldres", "res_under_mask",
                        "mask_ws", "W", "h2_bf16", "res_lp", "xout_lp", "reserved"))


class KsLinMerge(C.Structure):
    _fields_ = _ptrs("part_m", "part_s", "part_c", "Wout", "g", "W2") + _ints("precision", "nblk", "C", "B")


class KsLinOut2(C.Structure):
    _fields_ = (_ptrs("X", "Wq", "W2", "bias", "Y", "Y2")
                + [("xb", C.c_int64), ("yb", C.c_int64), ("y2b", C.c_int64), ("wq_lo_off", C.c_int64)]
                + _ints("precision", "npix", "C", "B", "ldx", "x_coff", "ldy", "y_coff", "ldy2", "y2_coff", "x_lp", "y_lp", "hw", "rows"))


class KsLinCtx(C.Structure):
    _fields_ = (_ptrs("qkv", "part_m", "part_s", "part_c") + [("bstride", C.c_int64)]
                + _ints("ld", "n", "heads", "chunk", "nchunks", "B"))


class KsLinCombine(C.Structure):
    _fields_ = _ptrs("part_m", "part_s", "part_c", "Wout", "g", "Weff") + _ints("nchunks", "heads", "C", "B")


ATTN_PLANS = {"attention_direct_batch_regime": 0, "attention_direct_ksplit": 1, "attention_q64_ksplit": 2}
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not found: python -m dex_tts_amd.build builds it after the library")
    from dex_tts_amd import _lib as dexlib
    dexlib.load()                                     # torch's HIP runtime, then the library the shim links against
    lib = C.CDLL(LIB_PATH)
    lib.ks_struct_bytes.restype, lib.ks_struct_bytes.argtypes = C.c_int, [C.c_int]
    for k, T in enumerate((KsConv3, KsConvDown, KsConvTUp, KsAttn, KsRowChain, KsLinKvCtx, KsLinMerge, KsLinOut2, KsLinCtx, KsLinCombine)):
        if lib.ks_struct_bytes(k) != C.sizeof(T):
            raise RuntimeError(f"descriptor {T.__name__}: {C.sizeof(T)} bytes here, {lib.ks_struct_bytes(k)} in the shim")
    lib.ks_predicate.restype, lib.ks_predicate.argtypes = C.c_int, [C.c_int] * 8
    lib.ks_pack.restype = C.c_int
    lib.ks_pack.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p]
    lib.ks_attn_plan.restype, lib.ks_attn_plan.argtypes = C.c_int, [C.c_int] * 5
    for name, T in (("ks_conv3x3", KsConv3), ("ks_conv_down", KsConvDown), ("ks_convt_up", KsConvTUp), ("ks_attn_direct", KsAttn),
                    ("ks_attn_q64", KsAttn), ("ks_dit_rowchain", KsRowChain), ("ks_linattn_kvctx", KsLinKvCtx),
                    ("ks_linattn_merge", KsLinMerge), ("ks_linattn_out2", KsLinOut2), ("ks_linattn_ctx", KsLinCtx),
                    ("ks_linattn_combine", KsLinCombine)):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = C.c_int, [C.POINTER(T), C.c_void_p, C.c_char_p, C.c_int]
    lib.ks_conv3x3_strip_form.restype, lib.ks_conv3x3_strip_form.argtypes = C.c_int, [C.POINTER(KsConv3)]
    _lib = lib
    return lib


def _check(rc, what):
    if rc < 0:
        raise ShimError(f"{what}: rejected by the shim ({ERRORS.get(rc, rc)})")
    return rc


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def predicate(name, prec, *args):
    a = list(args) + [0] * (6 - len(args))
    return bool(_check(load().ks_predicate(PREDICATES[name], PREC[prec], *a), name))


def predicate_int(name, prec, *args):
    """A predicate that answers with a count (dit_rowchain_cluster_xcds)."""
    a = list(args) + [0] * (6 - len(args))
    return _check(load().ks_predicate(PREDICATES[name], PREC[prec], *a), name)


def _need(t, nbytes, name):
    """Tensor t (or None) as a pointer, after checking it is a contiguous device tensor of at least nbytes."""
    if t is None:
        return None
    if not (t.is_cuda and t.is_contiguous()):
        raise ShimError(f"{name}: not a contiguous device tensor")
    if t.numel() * t.element_size() < nbytes:
        raise ShimError(f"{name}: {t.numel() * t.element_size()} bytes, the descriptor implies {nbytes}")
    return t.data_ptr()


def pack(kind, w_kn, prec):
    """The library's packing of a device fp32 matrix: kind "nk" ([K][N] -> 16-bit [N][K]), "frag" ([K][N] -> MFMA fragment order),
    "frag_nk" (a [N][K] source -> the same fragment order: Wq of the linear attention's tail) or "cast" (the row-major 16-bit cast: Wkv
    of its context pass).  Returns (uint16 pack as an int16 tensor, lo_off): the split-weight mode's lo pack sits lo_off elements behind
    the hi pack, as dex_api.hip's pack3 lays it out."""
    K, N = w_kn.shape if kind != "frag_nk" else w_kn.shape[::-1]
    assert w_kn.is_cuda and w_kn.dtype == torch.float32 and w_kn.is_contiguous()
    split = prec == "fp16x2"
    lo_off = K * N if split else 0
    dst = torch.zeros(K * N * (2 if split else 1), dtype=torch.int16, device=w_kn.device)
    scratch = torch.zeros(K * N, dtype=torch.float32, device=w_kn.device) if split else None
    _check(load().ks_pack({"nk": 0, "frag": 1, "frag_nk": 2, "cast": 3}[kind], w_kn.data_ptr(), dst.data_ptr(), scratch.data_ptr() if split else None,
                          K, N, lo_off, PREC[prec], _stream()), f"pack {kind}")
    torch.cuda.current_stream().synchronize()         # (scratch is released on return)
    return dst, lo_off


def _conv3_desc(prec, t, H, W, Cin, Cout, B, ldx, x_coff, mask_ws, mask_bstride, step, row_bstride, x_bf16, y_bf16, xout_lp,
                w_lo_off, res_lo_off, res2_scal_stride, res2_planes):
    """t: dict of tensors by descriptor member name (absent / None = null)."""
    d = KsConv3()
    g = t.get
    npix = B * H * W
    last_row = step + (B - 1) * row_bstride
    split = 2 if prec == "fp16x2" else 1
    sizes = {
        "X": npix * ldx * (2 if x_bf16 else 4), "Y": npix * Cout * (2 if y_bf16 else 4), "bias": Cout * 4,
        "Wbf": (w_lo_off * (split - 1) + 9 * Cin * Cout) * 2, "Wfrag": (9 * Cin * Cout * split) * 2,
        "mask": ((B - 1) * mask_bstride + (W - 1) * mask_ws + 1) * 4,
        "pro_stats": B * 8 * GN_SLOTS * 2 * 8, "pro_gamma": Cin * 4, "pro_beta": Cin * 4, "pro_tadd": (last_row + 1) * Cin * 4,
        "pro_res": npix * Cin * 4, "pro_xout": npix * Cin * (2 if xout_lp else 4),
        "res2_w": max(res2_planes, 0) * 64 * 4, "res2_b": 64 * 4, "res2_mu": npix * 4, "res2_x": npix * 4, "res2_spk": B * H * 4,
        "res2_scal": (last_row * max(res2_scal_stride, 0) + 3) * 4,
        "res_w": (res_lo_off * (split - 1) + Cin * Cout) * 2, "res_wfrag": Cin * Cout * split * 2, "res_b": Cout * 4,
        "res_y": npix * Cout * 4, "gn_stats": B * 8 * GN_SLOTS * 2 * 8,
    }
    if step < 0 or row_bstride < 0 or min(H, W, B, Cin, Cout, ldx) <= 0:
        raise ShimError("conv3x3: negative or empty extent")
    for name, nbytes in sizes.items():
        setattr(d, name, _need(g(name), nbytes, name))
    for name in t:
        if name not in sizes:
            raise ShimError(f"conv3x3: unknown tensor {name}")
    d.mask_bstride, d.w_lo_off, d.res_lo_off = mask_bstride, w_lo_off, res_lo_off
    d.precision = PREC[prec]
    d.H, d.W, d.Cin, d.Cout, d.B, d.ldx, d.x_coff, d.mask_ws = H, W, Cin, Cout, B, ldx, x_coff, mask_ws
    d.step, d.row_bstride, d.x_bf16, d.y_bf16, d.xout_lp = step, row_bstride, int(x_bf16), int(y_bf16), int(xout_lp)
    d.res2_scal_stride, d.res2_planes = res2_scal_stride, res2_planes
    return d


def conv3x3(prec, tensors, *, H, W, Cin, Cout, B, ldx, x_coff=0, mask_ws=1, mask_bstride, step=0, row_bstride=0, x_bf16=False,
            y_bf16=False, xout_lp=False, w_lo_off=0, res_lo_off=0, res2_scal_stride=0, res2_planes=0, dry=False):
    """One launch_conv3x3_lp.  Returns the picked instantiation; dry=True launches nothing and returns whether the descriptor would
    run on a strip-walking form."""
    d = _conv3_desc(prec, tensors, H, W, Cin, Cout, B, ldx, x_coff, mask_ws, mask_bstride, step, row_bstride, x_bf16, y_bf16, xout_lp,
                    w_lo_off, res_lo_off, res2_scal_stride, res2_planes)
    if dry:
        return bool(_check(load().ks_conv3x3_strip_form(C.byref(d)), "conv3x3"))
    sym = C.create_string_buffer(128)
    _check(load().ks_conv3x3(C.byref(d), _stream(), sym, 128), "conv3x3")
    return sym.value.decode()


def _strip_desc(T, prec, t, names_w, *, H, W, B, Cc, ldx, x_coff, ldy, y_coff, a_lp, c_lp, inmask_ws, mask_bstride, Ho, Wo, taps):
    d = T()
    split = 2 if prec == "fp16x2" else 1
    if min(H, W, B, Cc, ldx, ldy) <= 0 or x_coff < 0 or y_coff < 0:
        raise ShimError("negative or empty extent")
    d.X = _need(t.get("X"), B * H * W * ldx * (2 if a_lp else 4), "X")
    d.Y = _need(t.get("Y"), B * Ho * Wo * ldy * (2 if c_lp else 4), "Y")
    d.bias = _need(t.get("bias"), Cc * 4, "bias")
    d.inmask = _need(t.get("inmask"), ((B - 1) * mask_bstride + (W - 1) * inmask_ws + 1) * 4, "inmask")
    for n in names_w:
        setattr(d, n, _need(t.get(n), taps * Cc * Cc * split * 2, n))
    d.xb, d.mask_bstride = H * W * ldx, mask_bstride
    d.precision, d.a_lp, d.c_lp, d.ldx, d.x_coff, d.H, d.W = PREC[prec], int(a_lp), int(c_lp), ldx, x_coff, H, W
    d.ldy, d.y_coff, d.inmask_ws, d.B, d.C = ldy, y_coff, inmask_ws, B, Cc
    return d


def conv_down(prec, tensors, *, H, W, B, ldx, x_coff=0, ldy, y_coff=0, a_lp=False, c_lp=False, inmask_ws=1, mask_bstride, Cc=64):
    d = _strip_desc(KsConvDown, prec, tensors, ["Wfrag"], H=H, W=W, B=B, Cc=Cc, ldx=ldx, x_coff=x_coff, ldy=ldy, y_coff=y_coff, a_lp=a_lp,
                    c_lp=c_lp, inmask_ws=inmask_ws, mask_bstride=mask_bstride, Ho=H // 2, Wo=W // 2, taps=9)
    sym = C.create_string_buffer(128)
    _check(load().ks_conv_down(C.byref(d), _stream(), sym, 128), "conv_down")
    return sym.value.decode()


def convt_up(prec, tensors, *, H, W, B, ldx, x_coff=0, ldy, y_coff=0, a_lp=False, c_lp=False, inmask_ws=1, mask_bstride, Cc=64):
    d = _strip_desc(KsConvTUp, prec, tensors, ["Wfrag0", "Wfrag1", "Wfrag2", "Wfrag3"], H=H, W=W, B=B, Cc=Cc, ldx=ldx, x_coff=x_coff,
                    ldy=ldy, y_coff=y_coff, a_lp=a_lp, c_lp=c_lp, inmask_ws=inmask_ws, mask_bstride=mask_bstride, Ho=2 * H, Wo=2 * W, taps=4)
    sym = C.create_string_buffer(128)
    _check(load().ks_convt_up(C.byref(d), _stream(), sym, 128), "convt_up")
    return sym.value.decode()


def attn_plan(name, prec, N, B, a=0):
    """The library's own attention plan functions: attention_direct_batch_regime(N, B), attention_direct_ksplit(N, B),
    attention_q64_ksplit(N, B, max_split)."""
    return _check(load().ks_attn_plan(ATTN_PLANS[name], PREC[prec], N, B, a), name)


def _attn(entry, prec, t, *, N, Npad, B, ksplit, o_sstride, o_lp, tail_g, tail_ks, half_g, half_n):
    """t: Qh, Kh, Vt (16-bit, fragment order), O (fp32 slots; 16-bit rows in slot 0 when o_lp), ml (or absent)."""
    if min(N, Npad, B) <= 0 or ksplit < 0 or tail_ks < 0 or o_sstride < 0:
        raise ShimError(f"{entry}: negative or empty extent")
    splits = max(ksplit, 1)
    slots = 1 + tail_ks if tail_ks > 1 else splits
    d = KsAttn()
    for n in ("Qh", "Kh", "Vt"):
        setattr(d, n, _need(t.get(n), B * 2 * Npad * 128 * 2, n))
        if t.get(n) is not None and t[n].dtype != LP_DTYPE[prec]:
            raise ShimError(f"{entry}: {n} is {t[n].dtype}, the mode's operands are {LP_DTYPE[prec]}")
    d.O = _need(t.get("O"), ((slots - 1) * o_sstride + B * N * 256) * 4, "O")
    d.ml = _need(t.get("ml"), max(splits, tail_ks) * B * 2 * N * 2 * 4, "ml")
    for n in t:
        if n not in ("Qh", "Kh", "Vt", "O", "ml"):
            raise ShimError(f"{entry}: unknown tensor {n}")
    d.o_sstride, d.N, d.Npad, d.B, d.ksplit, d.o_lp = o_sstride, N, Npad, B, ksplit, int(o_lp)
    d.tail_g, d.tail_ks, d.half_g, d.half_n, d.precision = tail_g, tail_ks, half_g, half_n, PREC[prec]
    form = C.create_string_buffer(192)
    _check(getattr(load(), entry)(C.byref(d), _stream(), form, 192), entry)
    return form.value.decode()


def attn_direct(prec, tensors, *, N, Npad, B, ksplit=1, o_sstride, o_lp=False, tail_g=0, tail_ks=0, half_g=0, half_n=0):
    """One launch_attention_direct.  Returns "attn_direct_kernel" or "attn_direct_ring_kernel xcd_map=<0|1>"."""
    return _attn("ks_attn_direct", prec, tensors, N=N, Npad=Npad, B=B, ksplit=ksplit, o_sstride=o_sstride, o_lp=o_lp, tail_g=tail_g,
                 tail_ks=tail_ks, half_g=half_g, half_n=half_n)


def attn_q64(prec, tensors, *, N, Npad, B, ksplit=1, o_sstride, o_lp=False, tail_g=0, tail_ks=0, half_g=0, half_n=-1):
    """One launch_attention_q64.  half_n < 0: whole units only, 0: the launcher's automatic half plan, > 0: forced.  Returns the
    plan launched: "attn_q64_kernel nunits=.. grid=.. ks=.. tail_g=.. tail_ks=.. half_g=.. half_n=.. xcd_mode=.."."""
    return _attn("ks_attn_q64", prec, tensors, N=N, Npad=Npad, B=B, ksplit=ksplit, o_sstride=o_sstride, o_lp=o_lp, tail_g=tail_g,
                 tail_ks=tail_ks, half_g=half_g, half_n=half_n)


def cluster_grid_tiles(prec, N, B, xlocal):
    """Clusters launch_dit_rowchain grids for: the row tiles, padded to whole rounds over the XCDs in use for XCD-local launches."""
    tiles = B * ((N + 31) // 32)
    if not xlocal:
        return tiles
    xc = predicate_int("dit_rowchain_cluster_xcds", prec, N, B)
    return (tiles + xc - 1) // xc * 8


def dit_rowchain(prec, t, *, B, N, Npad, ksplit=0, o_sstride=0, qkv_only=False, attn_inline=False, step=0, row_bstride=0, o_lp=False,
                 tail_row0=0, tail_ks=0, next_step_stride=0, qscale=1.0, epoch=0, xlocal=False):
    """One launch_dit_rowchain (DitChainP, csrc/kernels.h).  t: tensors by descriptor member name (absent / None = null): X fp32
    [B * N][256]; O fp32 slots (16-bit rows in slot 0 when o_lp), ml; Wp / W1 / W2 / Wq from pack("frag", ..) (the split mode's lo half
    behind the hi half); bp, b1, b2, bq; ada [steps][6 * 256]; next_shift / next_scale rows of next_step_stride floats; Qh / Kh / Vt
    (written) and Qin / Kin / Vin (read by the in-kernel attention), B * 2 * Npad * 128 16-bit each; xslab, and xflag whose last word
    is xerr.  Returns the instantiation the launcher picked."""
    if min(B, N, Npad) <= 0 or min(ksplit, tail_ks, tail_row0, o_sstride, step, row_bstride, next_step_stride, epoch) < 0:
        raise ShimError("dit_rowchain: negative or empty extent")
    split = 2 if prec == "fp16x2" else 1
    rows = step + (B - 1) * row_bstride + 1                  # rows of the conditioning tables the launch reads
    slots = 1 + tail_ks if tail_ks > 1 else max(ksplit, 1)
    opnd = B * 2 * Npad * 128 * 2
    gt = cluster_grid_tiles(prec, N, B, xlocal) if t.get("xflag") is not None else 0
    sizes = {"X": B * N * 256 * 4,
             "O": B * N * 256 * 2 if (o_lp and slots == 1) else ((slots - 1) * o_sstride + B * N * 256) * 4,
             "ml": max(ksplit, tail_ks) * B * 2 * N * 2 * 4,
             "Wp": 256 * 256 * split * 2, "W1": 256 * 512 * split * 2, "W2": 512 * 256 * split * 2, "Wq": 256 * 768 * split * 2,
             "bp": 256 * 4, "b1": 512 * 4, "b2": 256 * 4, "bq": 768 * 4, "ada": rows * 6 * 256 * 4,
             "next_shift": ((rows - 1) * next_step_stride + 256) * 4, "next_scale": ((rows - 1) * next_step_stride + 256) * 4,
             "Qh": opnd, "Kh": opnd, "Vt": opnd, "Qin": opnd, "Kin": opnd, "Vin": opnd,
             "xslab": B * ((N + 31) // 32) * DIT_CLUSTER_SLAB_FLOATS * 4, "xflag": (gt * DIT_CLUSTER_FLAG_WORDS + 1) * 4}
    d = KsRowChain()
    for name in t:
        if name not in sizes:
            raise ShimError(f"dit_rowchain: unknown tensor {name}")
    for name, nbytes in sizes.items():
        setattr(d, name, _need(t.get(name), nbytes, name))
    for n in ("Qh", "Kh", "Vt", "Qin", "Kin", "Vin"):
        if t.get(n) is not None and t[n].dtype != LP_DTYPE[prec]:
            raise ShimError(f"dit_rowchain: {n} is {t[n].dtype}, the mode's operands are {LP_DTYPE[prec]}")
    for n in ("X", "ml", "bp", "b1", "b2", "bq", "ada", "next_shift", "next_scale", "xslab"):
        if t.get(n) is not None and t[n].dtype != torch.float32:
            raise ShimError(f"dit_rowchain: {n} is {t[n].dtype}, not float32")
    d.o_sstride, d.next_step_stride = o_sstride, next_step_stride
    d.precision, d.B, d.N, d.Npad, d.ksplit, d.qkv_only, d.attn_inline = PREC[prec], B, N, Npad, ksplit, int(qkv_only), int(attn_inline)
    d.step, d.row_bstride, d.o_lp, d.tail_row0, d.tail_ks, d.xlocal = step, row_bstride, int(o_lp), tail_row0, tail_ks, int(xlocal)
    d.epoch, d.qscale = epoch, qscale
    form = C.create_string_buffer(128)
    _check(load().ks_dit_rowchain(C.byref(d), _stream(), form, 128), "dit_rowchain")
    return form.value.decode()


def _fill(d, entry, t, sizes, dtypes=None):
    """Descriptor pointers from the tensors t, each checked against the extent in sizes (bytes) and, where given, its dtype."""
    for name in t:
        if name not in sizes:
            raise ShimError(f"{entry}: unknown tensor {name}")
    for name, nbytes in sizes.items():
        setattr(d, name, _need(t.get(name), nbytes, name))
        want = (dtypes or {}).get(name)
        if want is not None and t.get(name) is not None and t[name].dtype not in (want if isinstance(want, tuple) else (want,)):
            raise ShimError(f"{entry}: {name} is {t[name].dtype}, not {want}")


def _run(entry, d):
    form = C.create_string_buffer(128)
    _check(getattr(load(), entry)(C.byref(d), _stream(), form, 128), entry)
    return form.value.decode()


def linattn_kvctx(prec, t, *, npix, C_, B, nsub, nblk, ldx=0, x_coff=0, xb=None, headwaves=False, rows=False, W=0, mask_ws=0,
                  mask_bstride=0, ldres=0, resb=None, res_under_mask=False, h2_bf16=False, res_lp=False, xout_lp=False, wkv_lo_off=0):
    """One launch_linattn_kvctx (LinKvCtxP, csrc/kernels.h).  t: X fp32 rows of ldx floats (non-PRO), or H2 / gn_stats / gamma / beta /
    mask / Xout and optionally res (the PRO form; X is not read); Wkv 16-bit [256][C] (the split mode's lo image wkv_lo_off elements
    behind); part_m / part_s [B][4][nblk][32], part_c [B][4][nblk][32][32].  Returns the instantiation, e.g.
    "linattn_kvctx_hw_kernel C=64 PRO=1 FL=5 ROWS=1"."""
    if min(npix, C_, B, nsub, nblk) <= 0 or min(ldx, x_coff, W, mask_ws, mask_bstride, ldres, wkv_lo_off) < 0:
        raise ShimError("linattn_kvctx: negative or empty extent")
    xb = npix * ldx if xb is None else xb
    resb = (npix * ldres if t.get("res") is not None else 0) if resb is None else resb
    split = prec == "fp16x2"
    f32, lp = torch.float32, LP_DTYPE[prec]
    sizes = {"X": ((B - 1) * xb + npix * ldx) * 4, "Wkv": ((wkv_lo_off if split else 0) + 256 * C_) * 2,
             "H2": B * npix * C_ * (2 if h2_bf16 else 4), "gn_stats": B * 8 * GN_SLOTS * 2 * 8, "gamma": C_ * 4, "beta": C_ * 4,
             "res": ((B - 1) * resb + npix * ldres) * (2 if res_lp else 4),
             "mask": ((B - 1) * mask_bstride + (max(W, 1) - 1) * mask_ws + 1) * 4,
             "part_m": B * 4 * nblk * 32 * 4, "part_s": B * 4 * nblk * 32 * 4, "part_c": B * 4 * nblk * 1024 * 4,
             "Xout": B * npix * C_ * (2 if xout_lp else 4)}
    d = KsLinKvCtx()
    _fill(d, "linattn_kvctx", t, sizes, {"X": f32, "H2": lp if h2_bf16 else f32, "res": lp if res_lp else f32, "mask": f32, "gamma": f32,
                                         "beta": f32, "gn_stats": torch.int64, "part_m": f32, "part_s": f32, "part_c": f32,
                                         "Xout": lp if xout_lp else f32, "Wkv": (torch.int16, lp)})
    d.xb, d.resb, d.mask_bstride, d.wkv_lo_off = xb, resb, mask_bstride, wkv_lo_off
    d.precision, d.npix, d.C, d.B, d.ldx, d.x_coff, d.nsub, d.nblk = PREC[prec], npix, C_, B, ldx, x_coff, nsub, nblk
    d.headwaves, d.rows, d.ldres, d.res_under_mask, d.mask_ws, d.W = int(headwaves), int(rows), ldres, int(res_under_mask), mask_ws, W
    d.h2_bf16, d.res_lp, d.xout_lp, d.reserved = int(h2_bf16), int(res_lp), int(xout_lp), 0
    return _run("ks_linattn_kvctx", d)


def linattn_merge(prec, t, *, nblk, C_, B):
    """One launch_linattn_merge.  t: part_m / part_s / part_c as the context pass writes them, Wout fp32 [C][128], g fp32 [1], W2 16-bit
    [B][C / 32][8][64][8] (written).  Returns "linattn_merge_kernel merge_fold<8 | 16 | 24>"."""
    if min(nblk, C_, B) <= 0:
        raise ShimError("linattn_merge: negative or empty extent")
    f32 = torch.float32
    sizes = {"part_m": B * 4 * nblk * 32 * 4, "part_s": B * 4 * nblk * 32 * 4, "part_c": B * 4 * nblk * 1024 * 4, "Wout": C_ * 128 * 4,
             "g": 4, "W2": B * C_ * 128 * 2}
    d = KsLinMerge()
    _fill(d, "linattn_merge", t, sizes, {"part_m": f32, "part_s": f32, "part_c": f32, "Wout": f32, "g": f32})
    d.precision, d.nblk, d.C, d.B = PREC[prec], nblk, C_, B
    return _run("ks_linattn_merge", d)


def linattn_out2(prec, t, *, npix, C_, B, ldx, x_coff=0, xb=None, ldy, y_coff=0, yb=None, ldy2=0, y2_coff=0, y2b=None, x_lp=False,
                 y_lp=False, hw=False, rows=False, wq_lo_off=0):
    """One launch_linattn_out2.  t: X (fp32, or the mode's 16-bit type when x_lp), Wq from pack("frag_nk", ..), W2 in the merge kernel's
    layout, bias fp32 [C] (g * b_out), Y (fp32, 16-bit when y_lp) and optionally Y2 (16-bit).  Returns the form: "linattn_out2_direct_kernel
    C=..", "linattn_out2_hw_kernel C=.. rows=..", or "linattn_out2_kernel C=.. (throughput)"."""
    if min(npix, C_, B, ldx, ldy) <= 0 or min(x_coff, y_coff, ldy2, y2_coff, wq_lo_off) < 0:
        raise ShimError("linattn_out2: negative or empty extent")
    xb = npix * ldx if xb is None else xb
    yb = npix * ldy if yb is None else yb
    y2b = (npix * ldy2 if t.get("Y2") is not None else 0) if y2b is None else y2b
    split = prec == "fp16x2"
    f32, lp = torch.float32, LP_DTYPE[prec]
    sizes = {"X": ((B - 1) * xb + npix * ldx) * (2 if x_lp else 4), "Wq": ((wq_lo_off if split else 0) + 128 * C_) * 2, "W2": B * C_ * 128 * 2,
             "bias": C_ * 4, "Y": ((B - 1) * yb + npix * ldy) * (2 if y_lp else 4), "Y2": ((B - 1) * y2b + npix * ldy2) * 2}
    d = KsLinOut2()
    _fill(d, "linattn_out2", t, sizes, {"X": lp if x_lp else f32, "bias": f32})
    d.xb, d.yb, d.y2b, d.wq_lo_off = xb, yb, y2b, wq_lo_off
    d.precision, d.npix, d.C, d.B, d.ldx, d.x_coff, d.ldy, d.y_coff = PREC[prec], npix, C_, B, ldx, x_coff, ldy, y_coff
    d.ldy2, d.y2_coff, d.x_lp, d.y_lp, d.hw, d.rows = ldy2, y2_coff, int(x_lp), int(y_lp), int(hw), int(rows)
    return _run("ks_linattn_out2", d)


def linattn_ctx(t, *, n, B, ld=384, bstride=None, chunk=512, nchunks=None, heads=4):
    """One launch_linattn_ctx (fp32 mode).  t: qkv fp32 rows of ld floats (q | k | v), part_m / part_s / part_c (written)."""
    if min(n, B, ld, chunk, heads) <= 0:
        raise ShimError("linattn_ctx: negative or empty extent")
    nchunks = (n + chunk - 1) // chunk if nchunks is None else nchunks
    bstride = n * ld if bstride is None else bstride
    f32 = torch.float32
    sizes = {"qkv": ((B - 1) * bstride + n * ld) * 4, "part_m": B * heads * nchunks * 32 * 4, "part_s": B * heads * nchunks * 32 * 4,
             "part_c": B * heads * nchunks * 1024 * 4}
    d = KsLinCtx()
    _fill(d, "linattn_ctx", t, sizes, {k: f32 for k in sizes})
    d.bstride, d.ld, d.n, d.heads, d.chunk, d.nchunks, d.B = bstride, ld, n, heads, chunk, nchunks, B
    return _run("ks_linattn_ctx", d)


def linattn_combine(t, *, nchunks, C_, B, heads=4):
    """One launch_linattn_combine (fp32 mode).  t: the partials, Wout fp32 [C][128], g fp32 [1], Weff fp32 [B][128][C] (written)."""
    if min(nchunks, C_, B, heads) <= 0:
        raise ShimError("linattn_combine: negative or empty extent")
    f32 = torch.float32
    sizes = {"part_m": B * heads * nchunks * 32 * 4, "part_s": B * heads * nchunks * 32 * 4, "part_c": B * heads * nchunks * 1024 * 4,
             "Wout": C_ * heads * 32 * 4, "g": 4, "Weff": B * heads * 32 * C_ * 4}
    d = KsLinCombine()
    _fill(d, "linattn_combine", t, sizes, {k: f32 for k in sizes})
    d.nchunks, d.heads, d.C, d.B = nchunks, heads, C_, B
    return _run("ks_linattn_combine", d)
