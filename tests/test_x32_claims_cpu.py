"""CPU: the ticket map of the 32x32 ONF kernel's tile claims (csrc/onf_x32_impl.h, "Tiles by claim"), as restated in
tools/x32/emulate_x32.py next to the address formulas.

A workgroup keeps the chunks it always owned (block + k grid < n_chunks) and hands their tiles out as tickets
0 .. K TPC - 1; a wave takes two tickets per claim -- claim c: t = 2 TPC (c / TPC) + c % TPC and t + TPC, one tile of two
consecutive owned chunks -- and leaves when the first one's chunk is past the last chunk.  Checked
here, for both workgroup shapes, grids of 1, 7 and 256 workgroups and every sample count of tests/test_gpu_k1_claim_bits.py
(with the 256-CU threshold T = 65536):
  * the pools of a launch hold every 32-sample tile of its chunks exactly once;
  * the kernel's exit test agrees with the pool size, for every ticket a claim can return;
  * a claim's second ticket past the pool maps to no sample below P (padding lanes), as does every ticket a late claim
    returns (each of the workgroup's waves overshoots once)."""
import importlib.util
import os

import pytest

from conftest import ROOT

T = 256 * 256
COUNTS = (1, 33, 64, 65, 255, 257, 1023, T, T + 1, T + 256 + 33, 2 * T - 31)


def _emu():
    spec = importlib.util.spec_from_file_location("emulate_x32", os.path.join(ROOT, "tools", "x32", "emulate_x32.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


emu = _emu()


@pytest.mark.parametrize("P", COUNTS)
@pytest.mark.parametrize("grid", (1, 7, 256))
@pytest.mark.parametrize("threads", (256, 512))
def test_pools_hold_every_tile_once_and_tickets_past_a_pool_are_padding(threads, grid, P):
    tpc = threads // 64
    ch = 32 * tpc
    n_chunks = (P + ch - 1) // ch
    grid = min(grid, n_chunks)             # launch_persistent: never more workgroups than chunks
    seen = []
    for block in range(grid):
        pool = emu.pool_tickets(P, threads, block, grid)
        assert pool > 0 and pool % tpc == 0
        waves = threads // 64
        # every claim that can happen: 0, 1, 2, ... until each wave has seen one past the pool
        n_claims = (pool // tpc + 1) // 2 * tpc
        for c in range(n_claims + waves):
            t0, t1 = emu.claim_tickets(c, threads)
            assert emu.claim_is_past_pool(c, P, threads, block, grid) == (t0 >= pool) == (c >= n_claims), (block, c, pool)
            for tk in (t0, t1):
                first = emu.ticket_first_sample(tk, threads, block, grid)
                if tk < pool:
                    assert t0 < pool       # a taken ticket belongs to an accepted claim
                    seen.append(first)
                else:
                    assert first >= P, (block, tk, first)     # no sample below P: padding lanes, nothing stored
        # the first TPC claims are one chunk wide: a launch with one chunk per workgroup starts every wave at once
        assert sorted(emu.claim_tickets(c, threads)[0] for c in range(tpc)) == list(range(tpc))
    assert sorted(seen) == list(range(0, n_chunks * ch, 32))      # every tile of every chunk, exactly once


@pytest.mark.parametrize("P", COUNTS)
def test_launch_shape_of_the_cases(P):
    """the cases sit on the shapes their names say: below the threshold 256 threads, from it on 512"""
    threads, grid = emu.launch_shape(P, cus=256)
    assert threads == (256 if P < T else 512)
    assert grid == min(256, (P + threads // 2 - 1) // (threads // 2))
