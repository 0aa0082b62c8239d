"""Invariants of the prepared streaming tables (mcs_prepare_*: TileHdr, row spans, descriptors).

The bytes an LDS-DMA chunk reads beyond what a pixel window uses never reach the mosaic, so no
comparison of outputs can see a chunk that leaves its camera frame.  These tests read the tables
back (Plan.tile_tables, after Plan.prepare -- which reads no frame byte) and restate the streaming
kernel's address arithmetic (wave_windows in csrc/mcs_kernels.hip) in NumPy:

  * every 16-byte chunk the kernel would enable lies inside its camera frame and inside the
    tile's LDS slot;
  * every pixel with a live tap reads two LDS windows that lie inside the slot (12-byte reads
    from the dword below the window) and inside the chunks their footprint row loads.
"""
import numpy as np
import pytest

import warp_edges as we

pytestmark = pytest.mark.gpu

DMA_WINDOW = 1024          # bytes of LDS one DMA instruction fills: 64 lanes x 16 bytes
WAVES = 8
JOBS_PER_WAVE = {1: 8, 2: 16}   # by TileHdr.fits


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    from multicamera_stitching_amd import _capi
    assert _capi.device_count() >= 1, "GPU tests need an MI355X (no HIP device visible)"


def check_tables(plan):
    """Asserts the invariants over every LDS-path tile of a prepared plan; returns the number of
    (chunks, windows) checked."""
    from multicamera_stitching_amd import _capi
    fd = plan.flat
    cn = fd.channels
    tiles, spans, desc = plan.tile_tables()
    n_tiles = spans.shape[0]
    st = plan.stats()
    assert n_tiles == st["tiles"]
    assert sum(1 for t in range(n_tiles) if tiles[t].fits == 0) == st["direct_tiles"]
    assert sum(1 for t in range(n_tiles) if tiles[t].fits == 2) == st["big_tiles"]
    bad = []
    n_chunks = n_windows = 0
    for t in range(n_tiles):
        h = tiles[t]
        if h.fits == 0:
            continue
        assert h.fits in (1, 2) and 0 <= h.ncam <= _capi.TILE_CAMS, (t, h.fits, h.ncam)
        assert h.buf_bytes % 16 == 0 and h.ring >= 2, (t, h.buf_bytes, h.ring)
        n_win_tile = 0
        slot = []      # per camera slot: (base, LDS pitch, rows, first job)
        for k in range(h.ncam):
            c = h.cam[k]
            pitch_f = fd.cam_w[c] * cn
            fbytes = pitch_f * fd.cam_h[c]
            rows = h.jobstart[k + 1] - h.jobstart[k]
            lpitch = h.stride[k] & 0xffff
            e = (h.last_shift >> (8 * k)) & 255
            assert rows >= 1 and lpitch >= 16 and lpitch % 128 == 0, (t, k, rows, lpitch)
            slot.append((h.base[k], lpitch, rows, h.jobstart[k]))
            n_win = (rows * lpitch + DMA_WINDOW - 1) // DMA_WINDOW
            n_win_tile += n_win
            # lane L of window w: LDS byte w * 1024 + 16 L of the slot -> footprint row, chunk
            off = (np.arange(n_win * 64, dtype=np.int64) * 16).reshape(n_win, 64)
            ri = off // lpitch
            ch = (off - ri * lpitch) >> 4
            sp = np.where(ri < rows, spans[t, h.jobstart[k] + np.minimum(ri, rows - 1)], 0)
            lo, n = sp & 0xff, (sp >> 8) & 0xff
            on = (ri < rows) & (ch >= lo) & (ch < lo + n)
            none = ~on.any(axis=1, keepdims=True)      # the window still issues: lane 0, chunk 0
            ch = np.where(none, 0, ch)
            on = on | (none & (np.arange(64) == 0))
            r = h.rmin[k] + np.minimum(ri, rows - 1)
            src = r * pitch_f + h.cal[k] - np.where(r == fd.cam_h[c] - 1, e, 0) + 16 * ch
            out = on & ((src < 0) | (src + 16 > fbytes))
            for w, lane in zip(*np.nonzero(out)):
                bad.append(f"tile {t} camera {c} row {int(r[w, lane])}: DMA chunk reads bytes "
                           f"{int(src[w, lane])}..{int(src[w, lane]) + 16} of a {fbytes}-byte frame")
            lds_end = h.base[k] + off + 16
            assert not (on & (lds_end > h.buf_bytes)).any(), (t, k, "DMA past the LDS slot")
            n_chunks += int(on.sum())
        assert n_win_tile <= JOBS_PER_WAVE[h.fits] * WAVES, (t, n_win_tile)
        # pixels with a live tap: both windows inside the slot and inside their row's chunks
        d = desc[t]
        live = (d[:, 1] | d[:, 2]) != 0
        for a in ((d[live, 0] & 0xffff).astype(np.int64), (d[live, 0] >> 16).astype(np.int64)):
            if not a.size:
                continue
            assert h.ncam >= 1, (t, "live pixels without a footprint")
            k = np.zeros(a.shape, np.int64)
            for kk in range(1, h.ncam):
                k = np.where(a >= slot[kk][0], kk, k)
            base = np.array([s[0] for s in slot])[k]
            lpitch = np.array([s[1] for s in slot])[k]
            rows = np.array([s[2] for s in slot])[k]
            job0 = np.array([s[3] for s in slot])[k]
            assert (a >= base).all() and (a <= h.buf_bytes - 12).all(), (t, "LDS window")
            ri = (a - base) // lpitch
            q = (a - base) - ri * lpitch
            assert (ri < rows).all(), (t, "window below its camera's footprint rows")
            sp = spans[t, job0 + ri].astype(np.int64)
            lo, n = 16 * (sp & 0xff), 16 * ((sp >> 8) & 0xff)
            assert ((q >= lo) & (q + 2 * cn <= lo + n)).all(), (t, "window outside its row span")
            n_windows += int(a.size)
    assert not bad, "%d chunks outside their frame, e.g. %s" % (len(bad), "; ".join(bad[:4]))
    return n_chunks, n_windows


@pytest.mark.parametrize("interp", [1, 0])
@pytest.mark.parametrize("name, ch", [(c["name"], ch) for c in we.CASES
                                      for ch in we.case_channels(c, (1, 3))])
def test_case_tables(name, ch, interp):
    case = we.BY_NAME[name]
    plan = we.case_plan(case, ch, interp)
    try:
        plan.prepare()
        n_chunks, n_windows = check_tables(plan)
        # (the tiny sources may have no tile left on the LDS path: that is what the check enforces)
        if not case.get("black") and not name.startswith("tiny_"):
            assert n_chunks > 0 and n_windows > 0
    finally:
        plan.close()


@pytest.mark.parametrize("ch", [1, 3])
def test_chain_tables(ch):
    """The 3-camera chain of odd pitches: the frames' last rows stream through the DMA shift."""
    plan, _, _ = we.chain_plan(ch)
    try:
        plan.prepare()
        tiles, _, _ = plan.tile_tables()
        assert any(tiles[t].last_shift for t in range(plan.stats()["tiles"]))
        n_chunks, n_windows = check_tables(plan)
        assert n_chunks > 0 and n_windows > 0
    finally:
        plan.close()


def test_dense_rig_tables():
    """Eight cameras 5 px apart, paste mode: the tiles that stay on the LDS path hold at most
    four cameras."""
    plan, _ = we.dense_plan()
    try:
        plan.prepare()
        n_chunks, n_windows = check_tables(plan)
        assert plan.stats()["direct_tiles"] > 0
    finally:
        plan.close()
