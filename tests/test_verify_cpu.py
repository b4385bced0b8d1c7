"""CPU tests of verify mode (no GPU needed).

* ``fra_plan_verify`` is declared, exported and bound; ``VerifyReport`` has the ABI's 32 bytes; null arguments are
  refused before the plan is looked at, so a stand-in pointer serves.
* ``tiles.mismatch_pixel`` maps a report's (window, first_sample, first_channel) to raster (row, col, band).
* ``make hostcheck``: the verify entry's argument validation in the stand-alone ASan + UBSan program.
* ``StreamEncoder(verify=True)`` over stubbed plans: a mismatching report and a decoder error each set their pyflac
  state, raise ``EncoderProcessException`` and let none of the call's frames reach the write callback.
"""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from flac_raster import _native as N
from flac_raster import tiles
from flac_raster.encoder import EncoderProcessException, EncoderState, StreamEncoder

ROOT = Path(__file__).resolve().parents[1]


def test_verify_is_declared_exported_and_bound():
    hdr = (ROOT / "include" / "flac_raster_amd.h").read_text()
    decl = set(re.findall(r"FRA_API\s+[^;(]*?\b(fra_\w+)\s*\(", hdr))
    L = N.load()
    assert "fra_plan_verify" in decl and "fra_plan_verify" in N.EXPORTS and hasattr(L, "fra_plan_verify")
    assert L.fra_abi_version() == 3
    assert C.sizeof(N.VerifyReport) == 32
    assert [f[0] for f in N.VerifyReport._fields_] == ["mismatches", "first_sample", "first_channel", "expected", "got",
                                                       "nframes"]
    assert N.VerifyReport.first_sample.offset == 8 and N.VerifyReport.nframes.offset == 28
    assert callable(N.Plan.verify) and issubclass(N.VerifyMismatch, N.NativeError)


def test_null_arguments_are_refused_without_a_gpu():
    L = N.load()
    plan = C.c_void_p(16)  # never dereferenced on these paths
    reports = (N.VerifyReport * 1)()
    bad = C.c_int32(5)
    assert L.fra_plan_verify(None, reports, C.byref(bad)) == -1 and b"null" in L.fra_last_error()
    assert L.fra_plan_verify(plan, None, C.byref(bad)) == -1 and b"null" in L.fra_last_error()
    assert L.fra_plan_verify(plan, reports, None) == -1 and b"null" in L.fra_last_error()
    assert bad.value == 5


def test_mismatch_pixel_on_ragged_windows():
    # (row_off, col_off, height, width): a ragged right-edge tile of 140 columns
    w = (0, 520, 300, 140)
    assert tiles.mismatch_pixel(w, 0, 0) == (0, 520, 0)
    assert tiles.mismatch_pixel(w, 139, 3) == (0, 659, 3)
    assert tiles.mismatch_pixel(w, 140, 1) == (1, 520, 1)
    assert tiles.mismatch_pixel(w, 100 * 140 + 139, 1) == (100, 659, 1)
    assert tiles.mismatch_pixel(w, 300 * 140 - 1, 2) == (299, 659, 2)
    # a ragged bottom-right corner tile; sample 4096 is the first of the second frame
    w = (256, 384, 44, 36)
    assert tiles.mismatch_pixel(w, 44 * 36 - 1, 0) == (299, 419, 0)
    assert tiles.mismatch_pixel((10, 20, 300, 260), 4095, 1) == (10 + 15, 20 + 195, 1)
    assert tiles.mismatch_pixel((10, 20, 300, 260), 4096, 7) == (10 + 15, 20 + 196, 7)
    # the pyflac shim's window: one row of n samples
    assert tiles.mismatch_pixel((0, 0, 1, 10000), 9999, 1) == (0, 9999, 1)
    # numpy integers (ctypes fields read back as Python ints, arrays do not)
    assert tiles.mismatch_pixel(np.array([2, 3, 5, 7]), np.int64(15), np.int32(2)) == (4, 4, 2)
    e = N.VerifyMismatch(3, (100, 659, 1), -5, 7, 2, 1)
    assert (e.tile, e.pixel, e.expected, e.got, e.mismatches) == (3, (100, 659, 1), -5, 7, 2)
    assert "tile 3" in str(e) and "row 100" in str(e) and "col 659" in str(e)


def test_raise_on_mismatch_names_the_first_bad_window():
    reps = (N.VerifyReport * 3)()
    for r in reps:
        r.first_sample = -1
    wins = [(0, 0, 300, 260), (0, 260, 300, 260), (0, 520, 300, 140)]
    N.raise_on_mismatch(list(reps), wins)  # clean: returns
    reps[1].mismatches, reps[1].first_sample, reps[1].first_channel, reps[1].expected, reps[1].got = 2, 261, 3, 11, -4
    reps[2].mismatches, reps[2].first_sample = 1, 0
    with pytest.raises(N.VerifyMismatch) as ei:
        N.raise_on_mismatch(list(reps), wins)
    e = ei.value
    assert (e.tile, e.pixel, e.expected, e.got, e.mismatches, e.bad_tiles) == (1, (1, 261, 3), 11, -4, 2, 2)


def test_host_check_program_covers_the_verify_entry():
    """make hostcheck: the host side of the device decoder, the verify entry's argument validation included, as a
    stand-alone program under AddressSanitizer + UBSan; no GPU."""
    csrc = ROOT / "flac-raster_amd" / "csrc"
    if not shutil.which("make") or not (shutil.which("hipcc") or Path("/opt/rocm/bin/hipcc").exists()):
        pytest.skip("no make / hipcc")
    assert "fra_internal_verify_device" in (ROOT / "tools" / "decode_host_check.cpp").read_text()
    subprocess.run(["make", "-C", str(csrc), "hostcheck"], check=True, capture_output=True)
    run = subprocess.run([str(csrc / "build" / "decode_host_check"), str(ROOT / "tests" / "golden" / "sample_rgb.flac")],
                         capture_output=True, text=True)
    assert run.returncode == 0 and "argument validation checked" in run.stdout and "host check ok" in run.stdout, \
        run.stdout[-4000:] + run.stderr[-4000:]


# ----------------------------------------------------------------------------------- StreamEncoder(verify=True)
class _StubPlan(N.Plan):
    """A plan without a device: ``encode_host`` writes 10 bytes per frame; ``verify`` is ``Plan.verify`` (patched)."""

    def __init__(self, n, bs):
        self.n, self.bs, self.h, self.nwin = n, bs, None, 1
        self.calls = []

    def set_first_frame(self, k):
        self.calls.append(("first", k))

    def encode_host(self, raster, out):
        nfr = -(-self.n // self.bs)
        out[:10 * nfr] = np.arange(10 * nfr, dtype=np.uint8)
        self.calls.append(("encode", len(raster)))
        return 10 * nfr

    def frame_offsets(self, nfr):
        return np.arange(nfr + 1, dtype=np.uint64) * 10

    def close(self):
        pass


def _stub_encoder(monkeypatch, verify, bs=256):
    got = []
    enc = StreamEncoder(44100, lambda buf, nbytes, nsamp, frame: got.append((bytes(buf), nsamp, frame)),
                        compression_level=5, blocksize=bs, verify=verify)
    plans = {}

    def plan_for(n):
        if n not in plans:
            plans[n] = (_StubPlan(n, bs), np.zeros(10 * (n // bs + 2), np.uint8))
        return plans[n]

    monkeypatch.setattr(enc, "_plan_for", plan_for)
    monkeypatch.setattr(enc, "close", lambda: None)
    return enc, got, plans


def _report(mismatches=0, first_sample=-1, first_channel=0, expected=0, got=0, nframes=0):
    r = N.VerifyReport()
    r.mismatches, r.first_sample, r.first_channel, r.expected, r.got, r.nframes = (
        mismatches, first_sample, first_channel, expected, got, nframes)
    return r


def test_stream_encoder_verify_mismatch(monkeypatch):
    bs = 256
    a = (np.arange(3 * bs * 2, dtype=np.int16) % 97).reshape(-1, 2)
    verdicts = [_report(nframes=2), _report(3, 100, 1, 12, -7, 1)]
    seen = []

    def verify(self):
        seen.append(self.n)
        return [verdicts[len(seen) - 1]]

    monkeypatch.setattr(N.Plan, "verify", verify)
    enc, got, plans = _stub_encoder(monkeypatch, True)
    enc.process(a[:2 * bs + 1])  # two blocks are encoded (one sample of look-ahead), verified clean and emitted
    assert seen == [2 * bs] and enc.state == EncoderState.OK
    assert [(n, f) for _, n, f in got] == [(0, 0)] * 3 + [(bs, 0), (bs, 1)]
    emitted = len(got)
    with pytest.raises(EncoderProcessException, match="VERIFY_MISMATCH_IN_AUDIO_DATA") as ei:
        enc.process(a[2 * bs + 1:])  # buffered: nothing to encode yet
        enc.finish()  # the last block: verify reports a mismatch
    assert seen == [2 * bs, bs]
    assert enc.state == EncoderState.VERIFY_MISMATCH_IN_AUDIO_DATA
    assert len(got) == emitted, "a frame of the failing call reached the write callback"
    # the message names the stream's sample (two blocks emitted before), the channel and both values
    msg = str(ei.value)
    assert f"sample {2 * bs + 100}" in msg and "channel 1" in msg and "expected 12" in msg and "got -7" in msg
    assert any(c[0] == "encode" for c in plans[bs][0].calls)  # the encode did run before the verify


def test_stream_encoder_verify_decoder_error(monkeypatch):
    bs = 256

    def verify(self):
        raise N.NativeError("flac_raster_amd error -1: lost sync / corrupt frame at byte 40")

    monkeypatch.setattr(N.Plan, "verify", verify)
    enc, got, _ = _stub_encoder(monkeypatch, True)
    a = np.zeros((bs + 5, 1), np.int32)
    with pytest.raises(EncoderProcessException, match="corrupt frame at byte 40"):
        enc.process(a)
    assert enc.state == EncoderState.VERIFY_DECODER_ERROR
    assert [(n, f) for _, n, f in got] == [(0, 0)] * 3  # the stream header only


def test_stream_encoder_without_verify_never_asks(monkeypatch):
    bs = 256

    def verify(self):
        raise AssertionError("verify=False must not verify")

    monkeypatch.setattr(N.Plan, "verify", verify)
    enc, got, _ = _stub_encoder(monkeypatch, False)
    enc.process(np.zeros((2 * bs + 9, 2), np.int16))
    enc.finish()
    assert [(n, f) for _, n, f in got][3:] == [(bs, 0), (bs, 1), (9, 2)]
    # and with verify on and clean reports, the callback sequence and bytes are the same
    monkeypatch.setattr(N.Plan, "verify", lambda self: [_report(nframes=1)])
    enc2, got2, _ = _stub_encoder(monkeypatch, True)
    enc2.process(np.zeros((2 * bs + 9, 2), np.int16))
    enc2.finish()
    assert got2 == got


def test_cli_reports_a_verify_mismatch_and_exits_1(tmp_path, monkeypatch):
    from typer.testing import CliRunner

    from flac_raster import cli, streaming

    src = tmp_path / "scene.tif"
    src.write_bytes(b"II*\x00")
    asked = []

    def create(input_path, output_path, tile_size, level, devices, verify=False):
        asked.append(verify)
        raise N.VerifyMismatch(7, (300, 419, 2), 1234, -77, 3, 2)

    monkeypatch.setattr(streaming, "create_streaming_flac", create)
    res = CliRunner().invoke(cli.app, ["convert", str(src), "-o", str(tmp_path / "o.flac"), "--streaming", "--verify"])
    assert res.exit_code == 1 and asked == [True]
    out = " ".join(res.output.split())
    assert "tile 7" in out and "row 300 col 419 band 2" in out and "1234" in out and "-77" in out
    # --verify belongs to the TIFF -> FLAC directions
    flac = tmp_path / "x.flac"
    flac.write_bytes(b"fLaC")
    res = CliRunner().invoke(cli.app, ["convert", str(flac), "-o", str(tmp_path / "o.tif"), "--verify"])
    assert res.exit_code == 1 and "--verify" in res.output


def test_distributed_encode_passes_verify_to_every_rank():
    """``encode_tiles_distributed(verify=True)``: each rank's encode call gets ``verify=True`` beside its frame ranges
    (so a rank verifies its own ranged plan); without it the call is what it was."""
    from flac_raster.dist import encode_tiles_distributed

    class Rank:  # stands in for dist.Dist: rank 1 of 2, not the writer
        world, rank, local_rank = 2, 1, 1

        def gather_streams(self, items, dst=0):
            self.sent = items

    tls = tiles.calculate_tiles(300, 420, 128)
    calls = []

    def encode_fn(raster, my_tiles, level, devices, **kw):
        calls.append((len(my_tiles), devices, kw))
        return [None] * len(my_tiles)

    r = np.zeros((1, 300, 420), np.uint16)
    assert encode_tiles_distributed(r, tls, 5, Rank(), encode_fn=encode_fn, verify=True) is None
    assert encode_tiles_distributed(r, tls, 5, Rank(), encode_fn=encode_fn) is None
    (n1, dev1, kw1), (n2, dev2, kw2) = calls
    assert n1 == n2 > 0 and dev1 == dev2 == [1]
    assert kw1.get("verify") is True and "verify" not in kw2
    assert "frame_ranges" in kw1 and kw1["frame_ranges"] == kw2["frame_ranges"]
