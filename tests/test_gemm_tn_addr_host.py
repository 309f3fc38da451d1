"""CPU check of the address-free read phase of the 16-row TN main loop (csrc/gemm.hip, gemm_pers_kernel: frag16_tr_off, pair16s, run_units_tn; compiled with
-DGEMM_M16=7).  The kernel forms 8 + 4 lane addresses once per item (fragment 0 of each k-strided image with the fragment index XORed into bits 5..7) and
reaches ring slot, second transpose read and paired geometry through constants.  Restated here and checked exhaustively, in the style of
tests/test_gemm_m16_layout.py: for every lane, ring slot, fragment and image geometry
  (a) pinned address + half-of-the-ring scalar + immediate == ring slot origin + image origin + the address frag16<false> computes (ks_addr, the restatement
      test_gemm_m16_layout.py already pins to the DMA placement),
  (b) the immediate fits the 16-bit offset field of a ds_read and the read stays inside its image,
  (c) each transpose read is bank-conflict-free per 32-lane half (so also per 16-lane service group),
  (d) the DMA slot written out in pair16s is the slot issue_lo / issue_hi would have used, and run_units_tn visits (slot, REM) exactly as run_units does."""
from test_gemm_m16_layout import ks_addr

UNIT = 40960                        # ring slot (gemm.hip)
# (operand, rows_log2, image origin inside the slot, fragments per wave, row-origin step of the waves): full tile and paired item
GEOMETRIES = [("A", 8, 0, 8, 128), ("A", 9, 0, 8, 128), ("B", 8, 16384, 4, 64), ("B", 7, 32768, 4, 64)]


def pinned(r0, lane, rows_log2, origin, j):          # gemm.hip: fa[i] = frag16_tr_off(a_rb, ...) ^ (i << 5); fb[j] = (boff + frag16_tr_off(b_rb, ...)) ^ (j << 5)
    return (origin + ks_addr(r0, lane, rows_log2, 0)[2]) ^ (j << 5)


def read_addr(r0, lane, rows_log2, origin, j, slot, e):   # pair16s: q = smem + (f + roff); lds_tr_read(q + SO [+ AE / BE])
    roff, u = (slot >> 1) * 2 * UNIT, slot & 1
    imm = u * UNIT + e * (4 << (rows_log2 + 1))
    return pinned(r0, lane, rows_log2, origin, j) + roff, imm


def test_pinned_address_plus_immediate_is_the_fragment_address():
    for _, rl, origin, nfrag, step in GEOMETRIES:
        image_bytes = 32 << (rl + 1)
        for r0 in range(0, 1 << rl, step):
            for lane in range(64):
                for j in range(nfrag):
                    for slot in range(4):
                        for e in (0, 1):
                            base, imm = read_addr(r0, lane, rl, origin, j, slot, e)
                            want = ks_addr(r0 + 16 * j, lane, rl, e)[2]
                            assert base + imm == slot * UNIT + origin + want, (rl, r0, lane, j, slot, e)
                            assert 0 <= imm < 1 << 16
                            assert 0 <= want and want + 8 <= image_bytes and origin + image_bytes <= UNIT


def test_reads_stay_conflict_free():
    for _, rl, origin, nfrag, step in GEOMETRIES:
        for r0 in range(0, 1 << rl, step):
            for j in range(nfrag):
                for slot in range(4):
                    for e in (0, 1):
                        for half in (0, 1):           # ds_read_b64_tr_b16: 32 lanes x 2 banks
                            banks = []
                            for lane in range(32 * half, 32 * half + 32):
                                base, imm = read_addr(r0, lane, rl, origin, j, slot, e)
                                banks += [((base + imm) // 4) % 64, ((base + imm) // 4 + 1) % 64]
                            assert sorted(banks) == list(range(64)), (rl, r0, j, slot, e, half)
                            for q in range(2):        # the 16-lane service groups of that half
                                g = banks[32 * q:32 * q + 32]
                                assert len(set(g)) == 32


def run_units(nk):                                   # gemm.hip run_units: (ring slot, units that follow, capped at 3) per unit
    seq, t = [], 0
    while t < nk - 3:
        seq.append((t & 3, 3)); t += 1
    if nk >= 3:
        seq.append((t & 3, 2)); t += 1
    seq.append((t & 3, 1)); t += 1
    seq.append((t & 3, 0))
    return seq


def run_units_tn(nk):                                # gemm.hip run_units_tn / pair16s, with the DMA slot of every issuing unit
    seq, dma, left, roff = [], [], nk, 0

    def pair(rem0):
        for u in (0, 1):
            rem = rem0 - u
            slot = (roff // UNIT) + u
            seq.append((slot, min(rem, 3)))
            if rem >= 3:
                ds = ((roff ^ (2 * UNIT)) + UNIT) if u == 0 else roff
                dma.append((slot, ds))
    while left >= 6:
        pair(4); left -= 2; roff ^= 2 * UNIT
    if left == 4:
        pair(3); roff ^= 2 * UNIT
    pair(1)
    return seq, dma


def test_pairs_visit_slots_and_waits_as_the_single_units_do():
    for nk in range(2, 42, 2):                       # k ranges are multiples of 64: an item has an even number of 32-deep units
        seq, dma = run_units_tn(nk)
        assert seq == run_units(nk), nk
        for slot, ds in dma:                         # unit t issues the pieces of unit t + 3 into slot (t + 3) & 3
            assert ds == ((slot + 3) & 3) * UNIT, (nk, slot, ds)
