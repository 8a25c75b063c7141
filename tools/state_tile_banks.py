#!/usr/bin/env python3
"""LDS bank arithmetic of the state kernels' tile (gcm_amd/csrc/kernels_state.hip,
DESIGN.md §3.6.2), enumerated: every lane group of every LDS instruction of
k_state_pack<M> and k_state_unpack<M>, M = 2, 3, 4, 5, 9.

A double at tile index i covers dwords 2 i and 2 i + 1.  An access is free of
bank conflicts when
  * the indices of each group of 16 consecutive lanes differ modulo 16
    (ds_write_b64 and each half of a ds_*2_b64: dword modulo 32), and
  * the indices of each group of 32 lanes differ modulo 32 (ds_read_b64: dword
    modulo 64).
Both are asked of both sides of the tile (the AoS side, lane l at e = l + 64 k;
the plane side, lane l at e = l M + c), so the answer holds for whichever form
the compiler picks.  Also shows that padding alone does not do it for even M.

    python tools/state_tile_banks.py        # exits 1 on a conflict
"""
import sys

MS = (2, 3, 4, 5, 9)


def slot(M, e):
    """tile_slot<M> of kernels_state.hip."""
    if M % 2:
        return e
    j = e >> 4
    r = j + (j >> 1) if M == 2 else j + (j >> 2)
    return (e & ~15) | ((e + r) & 15)


def conflict_free(M, index):
    sides = [[[l + 64 * k for l in range(64)] for k in range(M)],   # AoS side
             [[l * M + c for l in range(64)] for c in range(M)]]    # plane side
    for side in sides:
        for lanes in side:
            for width in (16, 32):
                for g in range(0, 64, width):
                    if len({index(e) % width for e in lanes[g:g + width]}) != width:
                        return False
    return True


def main():
    ok = True
    for M in MS:
        inj = len({slot(M, e) for e in range(64 * M)}) == 64 * M and max(slot(M, e) for e in range(64 * M)) < 64 * M
        free = conflict_free(M, lambda e: slot(M, e))
        print(f"M = {M}: slot() a permutation of the tile: {inj}; conflict-free in both directions: {free}")
        ok = ok and inj and free
    for M in (2, 4):
        rows = [S for S in range(64, 200) if conflict_free(M, lambda e: (e % M) * S + e // M)]
        pads = [(Q, P) for Q in (16, 32, 64) for P in range(8) if conflict_free(M, lambda e: e + (e // Q) * P)]
        print(f"M = {M}: row strides 64..199 of a [component][node] tile that work: {rows}; "
              f"pads of P < 8 doubles every Q in (16, 32, 64) elements that work: {pads}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
