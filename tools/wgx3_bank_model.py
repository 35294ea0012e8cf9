"""LDS bank model of conv_wgrad_tile_x3's pixel-major halo image (conv_f32.hip wgrad_x3_body).

python tools/wgx3_bank_model.py   (no GPU)
For CIB 32 (XH 8) and 64 (XH 4): every transposing A-fragment read (channel block of the wave,
wave row wr, shift s, read h, tile row kk, plane) and every staging store instruction (64
consecutive slots; the last one partly masked), by the rule of the 9-tap form: the lanes of a
32-lane half must fall on distinct banks (addr / 4) % 64, 8 bytes (two banks) per lane.
Prints the worst number of lanes per bank; 1 = conflict-free.
"""
TT_W, KS, NP = 16, 3, 3


def sw(cib, hx):
    return ((hx >> 3) & 1) | ((((hx >> 1) & 1) << 1) if cib == 64 else 0)


def worst(addrs):
    w = 0
    for half in (addrs[:32], addrs[32:]):
        banks = {}
        for a in half:
            assert a % 8 == 0
            for b in ((a // 4) % 64, (a // 4 + 1) % 64):
                banks[b] = banks.get(b, 0) + 1
        w = max([w] + list(banks.values()))
    return w


def model(cib, xh):
    hh, hw, pxb = xh + KS - 1, TT_W + KS - 1, cib * 2
    plb = hh * hw * pxb
    rd = 0
    for wci0 in range(0, cib, 32):
        for wr in range(3):
            for s in range(KS):
                for h in range(2):
                    for kk in range(xh):
                        for p in range(NP):
                            ad = []
                            for lane in range(64):
                                hx = 8 * (lane >> 5) + s + 4 * h + ((lane >> 2) & 3)
                                assert hx < hw and kk + wr < hh
                                blk = ((wci0 >> 4) + ((lane >> 4) & 1)) ^ sw(cib, hx)
                                ad.append(p * plb + ((kk + wr) * hw + hx) * pxb + (blk << 5) +
                                          8 * (lane & 3))
                            assert max(ad) + 8 <= NP * plb
                            rd = max(rd, worst(ad))
    st = 0
    xq = hh * hw * (cib // 4)
    for q0 in range(0, xq, 64):
        ad = []
        for q in range(q0, min(q0 + 64, xq)):
            xcq, hp = q % (cib // 4), q // (cib // 4)
            ad.append(hp * pxb + (((xcq >> 2) ^ sw(cib, hp % hw)) << 5) + 8 * (xcq & 3))
        st = max(st, worst(ad))
    return rd, st


if __name__ == "__main__":
    for cib, xh in ((32, 8), (64, 4)):
        print("CIB %d XH %d: reads %d lane(s) per bank, stores %d" % ((cib, xh) + model(cib, xh)))
