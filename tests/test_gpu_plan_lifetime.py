"""GPU test of what a plan owns: plans created, used in every mode (pipelined executes, the host pipeline into a
pageable output, a host raster swap, a download) and closed, over and over, must give the same bytes every time and
must not lose device memory."""
import ctypes

import numpy as np
import pytest

from flac_raster import _native as N
from flac_raster.synth import synth_window
from flac_raster.tiles import calculate_tiles

pytestmark = pytest.mark.gpu

CYCLES = 10


@pytest.mark.parametrize("kind,bands,H,tile,dtype,level,norm,piped,wave", [
    (4, 1, 2048, 512, np.uint16, 5, 16, True, True),     # 1024 frames: pipelined, k_analyze_w
    (5, 2, 2048, 512, np.float32, 8, 24, True, False),   # a 32-bps plan
    (4, 1, 256, 128, np.uint16, 5, 16, False, True),     # not pipelined
])
def test_no_leak_across_plan_lifetimes(kind, bands, H, tile, dtype, level, norm, piped, wave):
    """After a warm-up cycle, CYCLES cycles of create, execute x3, sync, encode_host into a pageable array,
    set_raster from host, execute, download, close: equal bytes every cycle, and free device memory
    (hipMemGetInfo) drops by less than one plan.capacity() -- under a tenth of one output buffer per cycle."""
    hip = ctypes.CDLL("libamdhip64.so")  # the HIP runtime the product library runs on (one per process)

    def free_bytes():
        free, total = ctypes.c_size_t(), ctypes.c_size_t()
        assert hip.hipDeviceSynchronize() == 0
        assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value

    r = synth_window(kind, 17, bands, H, H).astype(dtype, copy=False)
    wins = calculate_tiles(H, H, tile)
    ctx = N.default_context(0)

    def cycle():
        plan = N.Plan(ctx, r.ctypes.data, False, r.dtype, bands, (H * H, H, 1), wins, level, 4096, norm, keepalive=r)
        try:
            assert bool(plan.flags() & 2) == piped and bool(plan.flags() & 4) == wave
            cap, _ = plan.capacity()
            for _ in range(3):
                plan.execute()
            plan.sync()
            page = np.empty(cap, np.uint8)
            total = plan.encode_host(r, page)
            plan.set_raster(r.ctypes.data, False, keepalive=r)
            plan.execute()
            _, frames = plan.download()
            return cap, page[:total].tobytes(), frames
        finally:
            plan.close()

    cap, first, frames = cycle()
    assert len(first) > 0 and frames == first
    before = free_bytes()
    for k in range(CYCLES):
        _, hosted, frames = cycle()
        assert hosted == first and frames == first, f"cycle {k}"
    after = free_bytes()
    print(f"free device memory: {before} -> {after} ({before - after:+d} bytes over {CYCLES} cycles; capacity {cap})")
    assert before - after < cap
