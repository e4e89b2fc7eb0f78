"""Plain-torch restatements of the layout kernels at the end of csrc/pointwise.hip: the operand packs, the weight-gradient unpacks, the
quad-form helpers and the two BatchNorm constant kernels.  Every function is fancy indexing (or a line of fp64 arithmetic) written from
the formulas of include/usseg.h ("operand packing", UssegBnFoldJob, the quad-form paragraph) - none walks tiles, workgroups or a flat
element index as the kernels do.  They run on whatever device their inputs live on; tests/test_cpu_layout_restatement.py checks them
against permutes, autograd and the oracle, tests/test_gpu_layout_routes.py checks the kernels against them.

A pack job is the tuple ops.pack_job builds: (src, dst, sT, sN, sK, T, Nn, Kk, Kw, tap_stride, n_off, k_off, reserved, nscale).
"""
import torch

J_SRC, J_DST, J_ST, J_SN, J_SK, J_T, J_NN, J_KK, J_KW, J_TAP, J_NOFF, J_KOFF, J_RES, J_NSCALE = range(14)
TILE = 32


def _tnk(T, Nn, Kk, device):
    """Index grids t, n, k of shape [T, Nn, Kk]."""
    return torch.meshgrid(torch.arange(T, device=device), torch.arange(Nn, device=device), torch.arange(Kk, device=device), indexing="ij")


# ------------------------------------------------------------------------------------------------ packs
def pack_dst_index(T, Nn, Kk, Kw, tap_stride, n_off, k_off, device="cpu"):
    """dst element index of (t, n, k): (n_off+n)*Kw + t*tap_stride + k_off + k, as a [T, Nn, Kk] tensor."""
    t, n, k = _tnk(T, Nn, Kk, device)
    return (n_off + n) * Kw + t * tap_stride + k_off + k


def pack_ref(src, sT, sN, sK, T, Nn, Kk, dst_shape, Kw, tap_stride, n_off, k_off, nscale=None):
    """src: the fp32 values from the job's src pointer on (any shape, read flat).  Returns (bf16 image of dst_shape, zero where nothing
    is written; boolean mask of the written positions).  Value: bf16_rne(fp32(src[t*sT+n*sN+k*sK]) * fp32(nscale[n])) - one fp32 multiply,
    one rounding, both reproduced exactly by torch, so a kernel is comparable bit for bit."""
    dev = src.device
    t, n, k = _tnk(T, Nn, Kk, dev)
    v = src.reshape(-1).float()[t * sT + n * sN + k * sK]
    if nscale is not None:
        v = v * nscale.reshape(-1).float()[n]           # indexed by n, not by n_off + n
    di = pack_dst_index(T, Nn, Kk, Kw, tap_stride, n_off, k_off, dev).reshape(-1)
    assert di.unique().numel() == di.numel(), "a pack job writes one destination element twice"
    numel = 1
    for s in dst_shape:
        numel *= s
    img = torch.zeros(numel, dtype=torch.bfloat16, device=dev)
    mask = torch.zeros(numel, dtype=torch.bool, device=dev)
    img[di] = v.reshape(-1).to(torch.bfloat16)
    mask[di] = True
    return img.reshape(dst_shape), mask.reshape(dst_shape)


def job_footprint(job, device="cpu"):
    """Sorted int64 tensor of the distinct destination element indices (relative to the job's dst pointer) one pack-job tuple writes."""
    di = pack_dst_index(int(job[J_T]), int(job[J_NN]), int(job[J_KK]), int(job[J_KW]), int(job[J_TAP]), int(job[J_NOFF]), int(job[J_KOFF]), device)
    return di.reshape(-1).unique()


def job_src_extent(job):
    """Number of floats from the src pointer a pack job can read: the largest t*sT + n*sN + k*sK, plus one."""
    return (int(job[J_T]) - 1) * int(job[J_ST]) + (int(job[J_NN]) - 1) * int(job[J_SN]) + (int(job[J_KK]) - 1) * int(job[J_SK]) + 1


def job_tiles(job):
    """Number of 32x32 tiles of a pack job: taps x 32-row blocks of n x 32-column blocks of k."""
    up = lambda v: -(-int(v) // TILE)
    return int(job[J_T]) * up(job[J_NN]) * up(job[J_KK])


def tilemap_ref(jobs, tiles_per_block):
    """The (job, first tile, tile count) triples of usseg_pack_weights_flat: each job's tiles cut into runs of tiles_per_block, the last
    run of a job ragged.  [nblocks, 3] int64."""
    trip = []
    for ji, job in enumerate(jobs):
        full, rest = divmod(job_tiles(job), tiles_per_block)
        trip += [(ji, b * tiles_per_block, tiles_per_block) for b in range(full)]
        if rest:
            trip.append((ji, full * tiles_per_block, rest))
    return torch.tensor(trip, dtype=torch.int64).reshape(-1, 3)


def tile_cover(jobs, tilemap):
    """Per job, how often the triples of `tilemap` ([nblocks,3] or flat) visit each of its tiles: a list of int64 count vectors.  A triple
    that names no job, leaves its job's tile range or has a count below 1 is an AssertionError."""
    tm = torch.as_tensor(tilemap).reshape(-1, 3).tolist()
    cover = [torch.zeros(job_tiles(j), dtype=torch.int64) for j in jobs]
    for ji, first, cnt in tm:
        assert 0 <= ji < len(jobs), f"triple names job {ji} of {len(jobs)}"
        assert cnt >= 1, f"triple ({ji}, {first}, {cnt}) has no tile"
        assert 0 <= first and first + cnt <= cover[ji].numel(), f"triple ({ji}, {first}, {cnt}) leaves the {cover[ji].numel()} tiles of its job"
        cover[ji][first:first + cnt] += 1
    return cover


# ------------------------------------------------------------------------------------------------ unpacks
def unpack_ref(scratch, Mrows, Ncols, T, Nn, Kk, n_off, k_off, dst0, sT, sN, sK, scale, accumulate):
    """dst[t*sT + n*sN + k*sK] (+)= scale * scratch[t][k_off+k][n_off+n].  dst0: what the destination held from the dst pointer on.
    Returns (expected fp64 values, magnitude |dst0| + |scale*scratch| (|scale*scratch| alone without accumulate), written mask), each of
    dst0's shape; outside the mask the expectation is dst0 itself."""
    dev = dst0.device
    t, n, k = _tnk(T, Nn, Kk, dev)
    s = float(torch.tensor(scale, dtype=torch.float32))          # the value the fp32 argument holds
    v = s * scratch.reshape(-1, Mrows, Ncols).double()[t, k_off + k, n_off + n].reshape(-1)
    di = (t * sT + n * sN + k * sK).reshape(-1)
    assert di.unique().numel() == di.numel(), "an unpack job writes one destination element twice"
    ref = dst0.reshape(-1).double().clone()
    mag = ref.abs()
    mask = torch.zeros(ref.numel(), dtype=torch.bool, device=dev)
    mask[di] = True
    if accumulate:
        ref[di] += v
        mag[di] += v.abs()
    else:
        ref[di] = v
        mag[di] = v.abs()
    return ref.reshape(dst0.shape), mag.reshape(dst0.shape), mask.reshape(dst0.shape)


# ------------------------------------------------------------------------------------------------ quad form
def quad_taps(k):
    """{(kh, kw): (stencil tap, parity class)} of the stride-2 'same' transposed convolution written as four parity-class convolutions:
    out[2i+a, 2j+b, n] = sum over source offsets (di, dj) of x[i+di, j+dj, :] . W[a+pad-2di][b+pad-2dj][n][:], pad = 0 (k = 3: out[2i'+kh] += x[i'] w[kh])
    or 1 (k = 4: out[2i'+kh-1] += ...), terms whose kernel index leaves [0, k) vanish.  A 3x3 'same' convolution reads x[i+di] at stencil row
    di+1, so (a, di) -> kernel row a+pad-2di, stencil row di+1; enumerated per axis, every kernel row must turn up exactly once."""
    assert k in (3, 4)
    pad = 1 if k == 4 else 0
    axis = {}
    for a in (0, 1):
        for d in (-1, 0, 1):
            kh = a + pad - 2 * d
            if 0 <= kh < k:
                assert kh not in axis
                axis[kh] = (a, d + 1)
    assert sorted(axis) == list(range(k))
    return {(kh, kw): (axis[kh][1] * 3 + axis[kw][1], axis[kh][0] * 2 + axis[kw][0]) for kh in range(k) for kw in range(k)}


def quad_weight(w, Np, Cin_phys=None):
    """Keras transposed-conv kernel [k,k,Cout,Cin] -> the quad-form 3x3 conv weight [9][Cin_phys][4*Np] (zero where no kernel tap lands)."""
    k, _, Cout, Cin = w.shape
    wq = torch.zeros(9, Cin_phys or Cin, 4 * Np, dtype=w.dtype, device=w.device)
    for (kh, kw), (t, cls) in quad_taps(k).items():
        wq[t, :Cin, cls * Np:cls * Np + Cout] = w[kh, kw].T
    return wq


def quad_unpack_ref(dq, Cin_phys, Cin, Cout, Np, k, grad0):
    """grad[kh][kw][n][c] = grad0 + dq[tap(kh,kw)][c][class(kh,kw)*Np + n], dq = [9][Cin_phys][4*Np].  fp64."""
    d = dq.reshape(9, Cin_phys, 4 * Np).double()
    ref = grad0.reshape(k, k, Cout, Cin).double().clone()
    for (kh, kw), (t, cls) in quad_taps(k).items():
        ref[kh, kw] += d[t, :Cin, cls * Np:cls * Np + Cout].T
    return ref


def quad_bias_expand_ref(bias, C, Np):
    """out[cls*Np + n] = bias[n] for n < C, 0 for the pad entries C <= n < Np; [4*Np], bias's dtype."""
    row = torch.zeros(Np, dtype=bias.dtype, device=bias.device)
    row[:C] = bias.reshape(-1)[:C]
    return row.repeat(4)


def quad_bias_fold_ref(d16, C, Np, dbias0):
    """dbias[n] = dbias0[n] + sum over the four parity classes of d16[cls*Np + n], n < C.  Returns (fp64 reference, magnitude), [C]."""
    d = d16.reshape(-1)[:4 * Np].double().reshape(4, Np)[:, :C]
    b0 = dbias0.reshape(-1)[:C].double()
    return b0 + d.sum(0), b0.abs() + d.abs().sum(0)


# ------------------------------------------------------------------------------------------------ BatchNorm constants
def bn_fold_ref(gamma, beta, mean, var, bias, C, Cp, eps):
    """scale = gamma*rsqrt(var+eps), shift = beta - mean*scale + scale*bias (bias may be None), zero for C <= c < Cp.
    Returns fp64 (scale, shift, |gamma|*rstd, |beta| + |mean*scale| + |scale*bias|), [Cp] each."""
    g, b, m, v = (t.reshape(-1)[:C].double() for t in (gamma, beta, mean, var))
    rstd = (v + float(torch.tensor(eps, dtype=torch.float32))).rsqrt()
    sc = g * rstd
    cb = bias.reshape(-1)[:C].double() if bias is not None else torch.zeros_like(sc)
    outs = (sc, b - m * sc + sc * cb, g.abs() * rstd, b.abs() + (m * sc).abs() + (sc * cb).abs())
    pad = lambda t: torch.cat([t, torch.zeros(Cp - C, dtype=torch.float64, device=t.device)])
    return tuple(pad(t) for t in outs)


def bn_finalize_ref(sum_, sumsq, M, momentum, mm0=None, mv0=None, stored=None):
    """mean = sum/M, var = max(sumsq/M - mean^2, 0) in fp64, with the magnitudes |sum|/M and sumsq/M + mean^2 (the two terms that cancel).
    With mm0 / mv0: the moving statistics moving*momentum + stat*(1-momentum), taken from `stored` = (mean, var) - the values the kernel
    itself stored - when given, and their magnitudes |moving|*momentum + |stat|*(1-momentum)."""
    s, s2 = sum_.double(), sumsq.double()
    mu = s / M
    r = dict(mean=mu, var=(s2 / M - mu * mu).clamp(min=0), mean_mag=s.abs() / M, var_mag=s2 / M + mu * mu)
    if mm0 is not None:
        mom = float(torch.tensor(momentum, dtype=torch.float32))
        smu, sv = (r["mean"], r["var"]) if stored is None else (stored[0].double(), stored[1].double())
        for key, m0, st in (("mm", mm0.double(), smu), ("mv", mv0.double(), sv)):
            r[key] = m0 * mom + st * (1 - mom)
            r[key + "_mag"] = m0.abs() * mom + st.abs() * (1 - mom)
    return r
