# CPU: the block -> work mapping of the production flash kernels
# (oobleck_amd/csrc/ob_flash_fold.h), queried through the host-only entries
# that call the very functions the kernels and launchers use.  An
# out-of-range row here would be an out-of-bounds access on the GPU, so this
# file is the gate before any GPU run of those kernels.
import ctypes

import pytest

FWD, DQ, DKDV = 0, 1, 2
KINDS = [FWD, DQ, DKDV]
SEQS = [128, 256, 384, 512, 640, 1024]
HEADS = [1, 3, 8, 12, 96]


def _ext():
    from oobleck_amd._ext import get_ext
    try:
        return get_ext()
    except RuntimeError as e:
        pytest.fail(f"extension must build on CPU via hipcc: {e}")


def _geom(kind, S):
    """(blocks per head, units per block, tile rows, tiles per sequence)"""
    if kind == DKDV:
        return S // 64, 2, 32, S // 32
    return S // 128, 4, 64, S // 64


def _rows(kind, S, block, unit):
    r0, t0, nt = ctypes.c_int64(-7), ctypes.c_int64(-7), ctypes.c_int64(-7)
    rc = _ext().ob_flash_fold_rows(kind, S, block, unit, ctypes.byref(r0),
                                   ctypes.byref(t0), ctypes.byref(nt))
    assert rc == 0, _ext().ob_last_error()
    return r0.value, t0.value, nt.value


@pytest.mark.parametrize("S", SEQS)
@pytest.mark.parametrize("kind", KINDS)
def test_rows_cover_sequence_once(kind, S):
    nblk, units, _, _ = _geom(kind, S)
    seen = [0] * S
    for blk in range(nblk):
        for u in range(units):
            r0, _, _ = _rows(kind, S, blk, u)
            assert r0 % 32 == 0
            assert 0 <= r0 and r0 + 32 <= S, (blk, u, r0)
            for r in range(r0, r0 + 32):
                seen[r] += 1
    assert seen == [1] * S


@pytest.mark.parametrize("S", SEQS)
@pytest.mark.parametrize("kind", KINDS)
def test_tile_ranges_hold_the_diagonal_and_nothing_past_it(kind, S):
    nblk, units, trows, ntile = _geom(kind, S)
    for blk in range(nblk):
        _, bt0, bnt = _rows(kind, S, blk, -1)
        # every staged tile lies inside the sequence
        assert 0 <= bt0 and bnt >= 1 and bt0 + bnt <= ntile, (blk, bt0, bnt)
        work = 0
        for u in range(units):
            r0, t0, nt = _rows(kind, S, blk, u)
            assert nt >= 1
            # the block stages every tile one of its units computes
            assert bt0 <= t0 and t0 + nt <= bt0 + bnt, (blk, u)
            if kind == DKDV:
                # q tiles from the one holding kv row r0 (its q rows
                # r0..r0+31 are the first with q >= kv) to the last
                assert t0 == r0 // 32
                assert t0 + nt == ntile
            else:
                # kv tiles 0 .. the one holding the unit's last row r0 + 31
                assert t0 == 0
                last = t0 + nt - 1
                assert last * trows <= r0 + 31 < (last + 1) * trows
            work += nt
        # the point of the fold: every block of a launch costs the same
        assert work == (ntile + 1 if kind == DKDV else 2 * ntile + 2)
        # ... and the block loop is exactly as long as its longest unit
        assert bnt == max(_rows(kind, S, blk, u)[2] for u in range(units))


@pytest.mark.parametrize("Z", HEADS)
@pytest.mark.parametrize("S", SEQS)
@pytest.mark.parametrize("kind", KINDS)
def test_id_map_hits_every_block_once(kind, S, Z):
    ext = _ext()
    nblk = _geom(kind, S)[0]
    grid = ext.ob_flash_fold_grid(kind, S, Z)
    assert grid == 8 * ((Z + 7) // 8) * nblk
    seen = {}
    pads = 0
    for i in range(grid):
        z, blk = ctypes.c_int64(-7), ctypes.c_int64(-7)
        ok = ext.ob_flash_fold_id(kind, S, Z, i, ctypes.byref(z),
                                  ctypes.byref(blk))
        assert 0 <= blk.value < nblk
        if ok:
            assert 0 <= z.value < Z
            assert (z.value, blk.value) not in seen
            seen[(z.value, blk.value)] = i
        else:
            assert z.value >= Z
            pads += 1
    assert len(seen) == Z * nblk
    assert pads == grid - Z * nblk
    # the blocks of one head share one residue class mod 8 (one XCD's L2)
    for z in range(Z):
        assert len({seen[(z, b)] % 8 for b in range(nblk)}) == 1


def test_rejects_bad_arguments():
    ext = _ext()
    a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    args = (ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    assert ext.ob_flash_fold_rows(FWD, 192, 0, 0, *args) != 0
    assert ext.ob_flash_fold_rows(FWD, 256, 2, 0, *args) != 0
    assert ext.ob_flash_fold_rows(DKDV, 256, 0, 2, *args) != 0
    assert ext.ob_flash_fold_rows(3, 256, 0, 0, *args) != 0
