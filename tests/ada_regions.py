"""Region arithmetic of the ADA geometric chain (test infrastructure; no kernel, no torch).

The chain (training/augment_mi.py:181-184 and :265-281) keeps a dynamically sized image at the origin of static
buffers.  Each kernel stores the logical image plus a band, and each consumer is trusted to read no further:

    forward    reflect_pad_dyn -> horizontal up-2 FIR -> vertical up-2 FIR -> affine_grid_sample(dyn_hw)
    backward   sampler gradient -> adjoint horizontal (down-2) FIR -> adjoint vertical FIR -> pad adjoint

The constants below mirror the kernels'; test_ada_geom_host.py reads the sources to hold the mirrors in place and
checks every producer / consumer pair, test_ada_geom_gpu.py builds its "as the producer leaves it" buffers from the
same regions.
"""
PAD_BAND = 64      # csrc/grid_sample.hip:204 reflect_pad_kernel: `min(Hs, Hd + 64), wl = min(Ws, Wd + 64)`
FIR_BAND = 32      # csrc/upfirdn2d.hip:53 `constexpr int kZeroBand = 32;` (the limited FIR passes)
GRAD_BAND = 96     # csrc/grid_sample.hip:309 `zero_region_kernel<<<...>>>(gin, p, dyn_hw, 96)` and :126 (the gather)
TAPS = 12          # setup_filter(wavelets['sym6']): augment_mi.py Hz_geom
UP_PAD0 = 6        # upsample2d_limited: p = [(fw + up - 1) // 2, (fw - up) // 2] = (6, 5)
ADJ_PAD0 = 5       # adjoint_params of that pass: fw - px0 - 1 = 5 (and 2 W - 2 W + 6 - 2 + 1 = 5 on the far side)


def lims(hd, wd):
    """The four (rows, cols) extents of upsample2d_limited: augment_mi.py:270-271 and csrc/augment.hip:133."""
    return [(hd + 32, 2 * wd + 32), (2 * hd + 32, 2 * wd + 32), (2 * hd + 96, wd + 32), (hd + 32, wd + 32)]


def reach(n_out, up, down, pad0, taps=TAPS):
    """One past the furthest input index that outputs 0 .. n_out - 1 of a FIR pass read: output o reads the
    zero-stuffed, padded positions u = o down - pad0 + t, t < taps, and u carries input u / up where up divides it."""
    return 0 if n_out <= 0 else ((n_out - 1) * down - pad0 + taps - 1) // up + 1


def support(n_in, up, down, pad0):
    """The first output index of a FIR pass all of whose taps lie at or beyond input index n_in: from there on the
    true output of an input supported on [0, n_in) is zero.  Output o's lowest input is ceil((o down - pad0) / up)."""
    return -(-(n_in * up + pad0) // down)


def clamp(region, buf):
    return (min(region[0], buf[0]), min(region[1], buf[1]))


def chain(h, w, margins):
    """-> dict name -> dict(buf, computed, written, support) per producer of the chain for an h x w image and
    margins (mx0, my0, mx1, my1); every region is (rows, cols), clamped to the static buffer.
    computed: where the producer stores values; written: computed plus its zero band; support: beyond it the true
    value is zero, so a zero band outside `support` is exact."""
    mx0, my0, mx1, my1 = margins
    hd, wd = h + my0 + my1, w + mx0 + mx1
    hs, ws = 3 * h - 2, 3 * w - 2
    l = lims(hd, wd)

    def stage(buf, computed, band, sup):
        return dict(buf=buf, computed=clamp(computed, buf), support=clamp(sup, buf),
                    written=clamp((computed[0] + band, computed[1] + band), buf))
    return dict(
        hd=hd, wd=wd, lims=l, dyn_hw=(2 * hd, 2 * wd),
        pad=stage((hs, ws), (hd, wd), PAD_BAND, (hd, wd)),
        fh=stage((hs, 2 * ws), l[0], FIR_BAND, (hd, support(wd, 2, 1, UP_PAD0))),
        fv=stage((2 * hs, 2 * ws), l[1], FIR_BAND, (support(hd, 2, 1, UP_PAD0), support(wd, 2, 1, UP_PAD0))),
        sg=stage((2 * hs, 2 * ws), (2 * hd, 2 * wd), GRAD_BAND, (2 * hd, 2 * wd)),
        ah=stage((2 * hs, ws), l[2], FIR_BAND, (2 * hd, support(2 * wd, 1, 2, ADJ_PAD0))),
        av=stage((hs, ws), l[3], FIR_BAND, (support(2 * hd, 1, 2, ADJ_PAD0), support(2 * wd, 1, 2, ADJ_PAD0))),
    )


def needs(ch):
    """-> list of (consumer, producer, rows, cols): one past the furthest row / column of the producer's buffer that
    the consumer's computed outputs read, clamped to the buffer (every kernel bounds-checks its taps against it)."""
    hd, wd = ch['hd'], ch['wd']
    fh, fv, ah, av = (ch[k]['computed'] for k in ('fh', 'fv', 'ah', 'av'))
    out = [
        ('fh', 'pad', fh[0], reach(fh[1], 2, 1, UP_PAD0)),          # a horizontal pass reads its own row
        ('fv', 'fh', reach(fv[0], 2, 1, UP_PAD0), fv[1]),           # a vertical pass its own column
        ('sampler', 'fv', 2 * hd, 2 * wd),                          # dyn_hw: corners outside it are skipped
        ('ah', 'sg', ah[0], reach(ah[1], 1, 2, ADJ_PAD0)),
        ('av', 'ah', reach(av[0], 1, 2, ADJ_PAD0), av[1]),
        ('pad_adjoint', 'av', hd, wd),                              # ys <= my0 + H - 1 + my1, xs likewise
    ]
    return [(c, p, *clamp((r, k), ch[p]['buf'])) for c, p, r, k in out]
