"""GPU: ordering and buffer lifetimes between the main stream and the look-ahead stream of the buffered overlap-mode driver
(`Cut3rSlam.run_buffered(pipeline=True)` -> `MotionFilter.prefetch_launch / prefetch_collect`).

Two hazards, each made deterministic instead of waiting for a race to go the wrong way:
  1. a device tensor the caller allocated on the main stream (a gathered image batch, a feature temporary) is consumed by the pass on the
     side stream and dropped by the caller as soon as `prefetch_launch` returns: the caching allocator must not hand its block out again
     before the side stream has read it;
  2. the encoder has static state (eager: the `enc...` buffers, graphs: static input and output of the captured pass): an encoder pass on the
     main stream must be ordered behind a pass in flight on the side stream.

How the race is decided: a bounded busy-wait (`torch.cuda._sleep`) is put on the side stream in front of the pass, so everything the test
then issues on the main stream finishes first -- every hazard test asserts that the pass was indeed still pending when the main stream had
drained (`not handle["event"].query()`), so none can pass because the delay was too short.  Every reference is the same call run
synchronously (`stream=None`) on a fresh filter; results are compared bit for bit.  Nothing here reads memory the allocator does not own,
and every wait is bounded by DELAY_MS."""
import gc
import os
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cut3r_slam_amd import synth  # noqa: E402
from cut3r_slam_amd.config import tiny_config  # noqa: E402
from cut3r_slam_amd.keyframe import KeyFrame  # noqa: E402
from cut3r_slam_amd.model import Cut3rModel  # noqa: E402
from cut3r_slam_amd.motion_filter import MotionFilter  # noqa: E402
from cut3r_slam_amd.slam import Cut3rSlam  # noqa: E402

DEV = "cuda:0"
H, W = 32, 48
NF = 24
MF = {"thresh": 0.9, "skip": 2, "kf_every": -1}
# The main-stream leg of a hazard test -- from the moment the busy-wait is enqueued: gather, issue the pass (host side), drop the temporary,
# fill the junk tensor, synchronise the main stream -- measured on an MI355X before the fixes: 0.25 - 0.47 ms once the side stream has run
# its first kernel (that one-off, 6 ms, is paid in the `side` fixture, outside every leg).  20 x the longest leg is 10 ms; the hold is set
# to 100 ms, 200 x the leg and half of the 200 ms that bound every wait in this file, so that a one-off host cost inside a leg (a garbage
# collection late in a long test process) does not decide the race either.  `hold_back` measures one hold and refuses to go on unless it
# lasted at least 20 x LEG_MS_MEASURED and at most 200 ms.
LEG_MS_MEASURED = 0.5
DELAY_MS = 100.0


def _model():
    cfg = tiny_config("dpt")
    return Cut3rModel(cfg, synth.tracking_state_dict(cfg, 3, enc_residual_gain=0.1), DEV, minimal=True)


def _filter(model, buffer=16):
    cfg = model.cfg
    kf = KeyFrame({}, (H, W), buffer, 2, DEV, feat_dim=cfg.enc_embed_dim, patch=cfg.patch_size)
    return MotionFilter(model, kf, dict(MF), DEV)


@pytest.fixture(scope="module")
def frames():
    return synth.slideshow_stream(NF, H, W, hold=3, seed=NF).to(DEV)      # frames 3k, 3k+1, 3k+2 share a texture


@pytest.fixture(scope="module")
def model():
    return _model()


@pytest.fixture(scope="module")
def feat0(model, frames):
    """encoder features of frame 0: the `last keyframe` every decision chain below starts from (computed once, never written)"""
    f = model.encode_batch(frames[0:1])[0].clone()
    torch.cuda.synchronize()
    return f


@pytest.fixture(scope="module")
def side():
    """the look-ahead stream of every test here (one stream: one placement on the hardware queues for the whole file), with its first
    kernel already behind it: what the first use of a stream costs is paid here, not inside a timed leg"""
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        torch.zeros(16, device=DEV).add_(1)
        torch.cuda._sleep(100_000)
    st.synchronize()
    torch.cuda.synchronize()
    return st


@pytest.fixture(scope="module")
def hold_back(side):
    """hold_back(stream): enqueue a busy-wait of DELAY_MS on `stream`.  Cycles per millisecond are calibrated once, with two events around
    one long _sleep on the side stream after a first one has brought the clocks up; then one hold is measured the same way and must lie
    between 20 x the leg and the 200 ms bound."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    probe = 60_000_000                                 # tens of milliseconds at any plausible counter rate
    with torch.cuda.stream(side):
        torch.cuda._sleep(probe)                       # loads the kernel, warms the clocks
        e0.record()
        torch.cuda._sleep(probe)
        e1.record()
    e1.synchronize()
    per_ms = probe / e0.elapsed_time(e1)
    cycles = int(DELAY_MS * per_ms)

    def hold(stream):
        with torch.cuda.stream(stream):
            torch.cuda._sleep(cycles)

    with torch.cuda.stream(side):
        e0.record()
    hold(side)
    with torch.cuda.stream(side):
        e1.record()
    e1.synchronize()
    held_ms = e0.elapsed_time(e1)
    print(f"[lookahead-streams] _sleep: {per_ms:.0f} cycles/ms, hold of {cycles} cycles measured {held_ms:.1f} ms (asked {DELAY_MS:.0f} ms)")
    assert 20 * LEG_MS_MEASURED <= held_ms <= 200.0, held_ms
    return hold


def _quiet():
    """before a timed leg: the device idle and the garbage collected, so that neither falls inside the leg"""
    torch.cuda.synchronize()
    gc.collect()


def _sync_pass(model, imgs, ts, forced, feat_last):
    """the reference of every test: the same call run synchronously on a fresh filter -> (features, host counts + decisions, kept)"""
    f = _filter(model)
    h = f.prefetch_launch(imgs, ts, list(forced), feat_last=feat_last, stream=None)
    kept, _ = f.prefetch_collect(h)
    torch.cuda.synchronize()
    return h["feats"].clone(), h["host"].clone(), kept


def _assert_pass_equals(h, kept, ref, what):
    feats, host, kept_ref = ref
    assert torch.equal(h["feats"], feats), f"{what}: features of the side-stream pass differ from the synchronous pass"
    assert torch.equal(h["host"], host), f"{what}: counts / decisions {h['host'].tolist()} != {host.tolist()}"
    assert kept == kept_ref, (what, kept, kept_ref)


def test_the_allocator_hands_a_freed_block_back_to_the_same_stream():
    """the precondition of the lifetime tests: a freed device tensor of the gather's size (and of the feature temporary's) is what the next
    allocation of that size on the same stream gets.  Only an allocator with caching switched off is excused."""
    if os.environ.get("PYTORCH_NO_HIP_MEMORY_CACHING") or os.environ.get("PYTORCH_NO_CUDA_MEMORY_CACHING"):
        pytest.skip("the caching allocator is switched off: no block is ever handed out twice")
    for shape, dtype in (((1, 3, H, W), torch.uint8), ((5, 3, H, W), torch.uint8), ((2, 3, H, W), torch.uint8), ((6, 64), torch.float32)):
        a = torch.empty(shape, dtype=dtype, device=DEV)
        p = a.data_ptr()
        del a
        b = torch.empty(shape, dtype=dtype, device=DEV)
        assert b.data_ptr() == p, (shape, dtype)


@pytest.mark.parametrize("idx,forced", [([4], [False]), ([1, 2, 4, 6, NF - 1], [False, False, False, False, True])], ids=["B1", "B5_forced_tail"])
def test_gathered_image_batch_outlives_the_caller(idx, forced, model, frames, feat0, hold_back, side):
    """The caller gathers `frames[idx]` on the main stream (what run_buffered's select() does for a chunk with always-kept frames), launches
    the pass on the side stream and drops the batch; the next main-stream allocation of that size is filled with 255.  While the pass is
    pending the allocator must not give that allocation the batch's block, and the pass must see the frames, not the 255s."""
    ts = list(idx)
    idx_t = torch.as_tensor(idx, device=DEV)
    ref = _sync_pass(model, frames[idx_t], ts, forced, feat0)
    f = _filter(model)
    f.prefetch_collect(f.prefetch_launch(frames[idx_t], ts, list(forced), feat_last=feat0))      # warm-up: capture, _chain_ws, _pos_grid
    _quiet()
    shape = (len(idx), 3, H, W)
    tic = time.perf_counter()
    hold_back(side)
    tmp = frames[idx_t]
    p = tmp.data_ptr()
    h = f.prefetch_launch(tmp, ts, list(forced), feat_last=feat0, stream=side)
    del tmp
    junk = torch.full(shape, 255, dtype=torch.uint8, device=DEV)
    torch.cuda.current_stream().synchronize()
    leg_ms = 1e3 * (time.perf_counter() - tic)
    pending = not h["event"].query()
    reused = junk.data_ptr() == p
    kept, _ = f.prefetch_collect(h)
    print(f"[lookahead-streams] image batch B={len(idx)}: leg {leg_ms:.2f} ms, pending {pending}, block reused {reused}, "
          f"features equal {torch.equal(h['feats'], ref[0])}, host {h['host'].tolist()} ref {ref[1].tolist()}")
    assert pending, "the side-stream pass finished before the main stream drained: the delay was too short to decide the race"
    assert not reused, "the gathered batch's block went to the next main-stream allocation while the side stream still had to read it"
    _assert_pass_equals(h, kept, ref, "gathered batch")
    assert int(junk.min()) == 255


def test_feat_last_temporary_outlives_the_caller(model, frames, feat0, hold_back, side):
    """the same for `feat_last`: the caller passes a clone of the chain's start features and drops it; the stand-in for the next main-stream
    allocation is a NaN-filled tensor of that size (a chain that started from NaNs matches no patch at all)."""
    idx, forced = [1, 2, 4, 6, 7], [False] * 5
    imgs = frames[torch.as_tensor(idx, device=DEV)]                       # held by the test until the end
    ref = _sync_pass(model, imgs, idx, forced, feat0)
    assert 0 < ref[1][5:].sum() < 5, "the reference chain keeps some frames and drops some"
    f = _filter(model)
    f.prefetch_collect(f.prefetch_launch(imgs, idx, list(forced), feat_last=feat0))
    _quiet()
    tic = time.perf_counter()
    hold_back(side)
    fl = feat0.clone()
    p = fl.data_ptr()
    h = f.prefetch_launch(imgs, idx, list(forced), feat_last=fl, stream=side)
    del fl
    junk = torch.full(tuple(feat0.shape), float("nan"), dtype=torch.float32, device=DEV)
    torch.cuda.current_stream().synchronize()
    leg_ms = 1e3 * (time.perf_counter() - tic)
    pending = not h["event"].query()
    reused = junk.data_ptr() == p
    kept, _ = f.prefetch_collect(h)
    print(f"[lookahead-streams] feat_last: leg {leg_ms:.2f} ms, pending {pending}, block reused {reused}, host {h['host'].tolist()} ref {ref[1].tolist()}")
    assert pending, "the side-stream pass finished before the main stream drained: the delay was too short to decide the race"
    assert not reused, "feat_last's block went to the next main-stream allocation while the side stream still had to read it"
    _assert_pass_equals(h, kept, ref, "feat_last temporary")
    assert bool(torch.isnan(junk).all())


def test_strided_view_batch_needs_no_protection(model, frames, feat0, hold_back, side):
    """CONTROL (passes before the fixes too): a regular chunk goes in as the strided view `frames[a:b:skip]` -- the caller makes no temporary,
    the contiguous copy is made on the side stream, by the side stream's allocator."""
    a, b, skip = 2, 12, 2
    ts = list(range(a, b, skip))
    forced = [False] * len(ts)
    ref = _sync_pass(model, frames[a:b:skip], ts, forced, feat0)
    f = _filter(model)
    f.prefetch_collect(f.prefetch_launch(frames[a:b:skip], ts, list(forced), feat_last=feat0))
    _quiet()
    hold_back(side)
    h = f.prefetch_launch(frames[a:b:skip], ts, list(forced), feat_last=feat0, stream=side)
    junk = torch.full((len(ts), 3, H, W), 255, dtype=torch.uint8, device=DEV)
    torch.cuda.current_stream().synchronize()
    pending = not h["event"].query()
    kept, _ = f.prefetch_collect(h)
    assert pending
    _assert_pass_equals(h, kept, ref, "strided view")
    assert int(junk.min()) == 255


@pytest.mark.parametrize("path", ["encode_batch", "window_features"])
@pytest.mark.parametrize("graphs", ["1", "0"], ids=["graphs", "eager"])
def test_main_stream_encodes_wait_for_the_pass_in_flight(graphs, path, monkeypatch, frames, hold_back, side):
    """The encoder's static state is shared by every pass of one batch size.  With a delayed pass of B images in flight on the side stream
    (asserted: still pending when the launch has returned), an encoder pass of B other images on the main stream -- `model.encode_batch`
    itself, or the product path: `TrackFrontend.window_features` with B stored keyframes whose features are missing -- must be ordered
    behind it: once the main stream has drained, the pass in flight is complete, and both sides have the features of their own images."""
    monkeypatch.setenv("CUT3R_GRAPHS", graphs)
    model = _model()
    assert model.use_graphs == (graphs == "1")
    B = 3
    ts = [2, 4, 6]
    forced = [False] * B
    view = frames[2:8:2]                                                  # the pass in flight: frames 2, 4, 6 (no temporary)
    other = frames[12:12 + B].contiguous()                                # the main stream's images, held by the test
    feat0 = model.encode_batch(frames[0:1])[0].clone()
    ref = _sync_pass(model, view, ts, forced, feat0)
    ref_other = model.encode_batch(other).clone()
    torch.cuda.synchronize()
    assert not torch.equal(ref_other, ref[0])
    if path == "encode_batch":
        f = _filter(model)
    else:                                                                 # keyframes 1, 3, 4 of a window of six have lost their features
        cfgd = {"Tracking": {"motion_filter": dict(MF), "frontend": {"iteration": 0}}}
        slam = Cut3rSlam(model, cfgd, (H, W), buffer=16, device=DEV)
        kf, f = slam.keyframes, slam.filterx
        intr = torch.tensor([40.0, 40.0, 23.5, 15.5])
        missing = [1, 3, 4]
        src = {1: 0, 3: 1, 4: 2}                                          # keyframe -> row of `other`
        filler = model.encode_batch(frames[9:10])[0].clone()
        for i in range(6):
            kf.append(float(i), other[src[i]] if i in src else frames[9], None, 1.0, None, None, intr, filler, None)
        for i in missing:
            kf.feat_valid[i] = False
    f.prefetch_collect(f.prefetch_launch(view, ts, list(forced), feat_last=feat0))      # warm-up: capture, _chain_ws, _pos_grid
    _quiet()
    hold_back(side)
    h = f.prefetch_launch(view, ts, list(forced), feat_last=feat0, stream=side)
    in_flight = not h["event"].query()
    if path == "encode_batch":
        got = model.encode_batch(other)
    else:
        slam.tracker.window_features(0, 6)
    torch.cuda.current_stream().synchronize()
    ordered = h["event"].query()
    kept, _ = f.prefetch_collect(h)
    torch.cuda.synchronize()
    if path == "window_features":
        got = torch.stack([kf.feat_slice(i, i + 1)[0] for i in missing])
    print(f"[lookahead-streams] {path} beside a pass in flight (graphs={graphs}): in flight {in_flight}, ordered {ordered}, "
          f"main equal {torch.equal(got, ref_other)}, side equal {torch.equal(h['feats'], ref[0])}")
    assert in_flight, "the side-stream pass had finished before the main-stream encode was issued: the delay was too short to decide the race"
    assert ordered, f"{path} encoded on the main stream while a side-stream pass of the same batch size was still in flight"
    assert torch.equal(got, ref_other), "main-stream features differ from the encode of those images alone"
    if path == "window_features":
        assert all(kf.feat_valid[i] for i in range(6))
        for i in (0, 2, 5):
            assert torch.equal(kf.feat_slice(i, i + 1)[0], filler)
    _assert_pass_equals(h, kept, ref, "pass in flight beside " + path)


@pytest.mark.parametrize("entry", ["encode", "prefetch"])
def test_filter_entry_points_wait_for_the_pass_in_flight(entry, model, frames, feat0, hold_back, side):
    """CONTROL (passes before the fixes too): `MotionFilter.encode` and `prefetch` have always waited for the filter's own pass in flight
    (asserted: still pending when the launch has returned)."""
    view = frames[4:5]
    ref = _sync_pass(model, view, [4], [False], feat0)
    other = frames[12:13]
    ref_other = model.encode_batch(other).clone()
    f = _filter(model)
    f.keyframes.append(0.0, frames[0], None, 1.0, None, None, torch.tensor([40.0, 40.0, 23.5, 15.5]), feat0, None)
    f.prefetch_collect(f.prefetch_launch(view, [4], [False], feat_last=feat0))
    _quiet()
    hold_back(side)
    h = f.prefetch_launch(view, [4], [False], feat_last=feat0, stream=side)
    in_flight = not h["event"].query()
    if entry == "encode":
        got = f.encode(other)[0]
    else:
        f.prefetch(other, [12], [False])
        got = f._ahead[12][0]
    torch.cuda.current_stream().synchronize()
    ordered = h["event"].query()
    kept, _ = f.prefetch_collect(h)
    torch.cuda.synchronize()
    assert in_flight, "the side-stream pass had finished before the entry point was called: the delay was too short to decide the race"
    assert ordered
    assert torch.equal(got, ref_other[0])
    _assert_pass_equals(h, kept, ref, "pass in flight beside MotionFilter." + entry)


def test_pipelined_driver_with_a_delayed_side_stream_equals_the_frame_by_frame_loop(hold_back, side):
    """Driver level: run_buffered(lookahead=5, pipeline=True) at skip 2 over 42 frames.  The chunk launched last (frames 40, 41: both always
    kept) is a gather chunk.  Every launch is held back on the look-ahead stream, and the next thing the main stream does after the launch
    has returned -- the first `run()` of the chunk being consumed -- is preceded by an allocation of the batch's shape filled with 255: the
    stand-in for the tracking windows' allocations.  (It cannot be made inside a wrapper of `prefetch_launch`: there the caller's argument
    still holds the batch.)  Keyframes, poses, depths, ordered edges and the stored encoder features are those of the frame-by-frame
    loop, bit for bit."""
    n, skip, lookahead = 42, 2, 5
    frames = synth.slideshow_stream(n, H, W, hold=3, seed=n).to(DEV)
    intr = torch.tensor([40.0, 40.0, 23.5, 15.5])
    model = _model()
    out = []
    # warm-up: one synchronous pass of each batch shape the look-ahead launches (5 tested frames; the 2 tail frames), so that no graph
    # capture -- it synchronises the device -- falls between a launch and the allocation that follows it
    model.encode_batch(frames[0:10:2])
    model.encode_batch(frames[n - 2:n])
    _quiet()
    seen = {"launches": 0, "gathers": 0, "pending": 0, "overlaps": 0, "junk": [], "todo": None}
    for drv in ("plain", "pipeline"):
        cfgd = {"Tracking": {"motion_filter": {"thresh": 0.9, "skip": skip, "kf_every": -1}, "frontend": {"iteration": 0, "window_batch": 1}}}
        slam = Cut3rSlam(model, cfgd, (H, W), buffer=n + 8, device=DEV)
        if drv == "plain":
            for t in range(n):
                slam.run(t, frames[t:t + 1], intr, frames[t:t + 1], intr, second_last_frame=(t == n - 2), last_frame=(t == n - 1))
        else:
            slam._ahead_stream = side
            launch, run = slam.filterx.prefetch_launch, slam.run

            def held_launch(images_u8, tstamps, forced=None, feat_last=None, stream=None):
                if stream is None:
                    return launch(images_u8, tstamps, forced, feat_last=feat_last)
                hold_back(stream)
                seen["launches"] += 1
                h = launch(images_u8, tstamps, forced, feat_last=feat_last, stream=stream)
                if images_u8.is_contiguous():                              # a gather: the caller's temporary
                    seen["gathers"] += 1
                    seen["todo"] = (tuple(images_u8.shape), images_u8.data_ptr(), images_u8.numel(), h)
                return h

            def run_after_junk(*a, **k):
                # fires exactly once: before the first `run()` of the chunk being consumed when the gather chunk was launched (held_launch
                # leaves `todo` only for a gather, and it is cleared here); every other call goes straight through
                if seen["todo"] is not None:
                    shape, p, nbytes, h = seen["todo"]
                    seen["todo"] = None
                    junk = torch.full(shape, 255, dtype=torch.uint8, device=DEV)
                    torch.cuda.current_stream().synchronize()
                    seen["junk"].append(junk)
                    seen["pending"] += int(not h["event"].query())
                    seen["overlaps"] += int(junk.data_ptr() < p + nbytes and p < junk.data_ptr() + nbytes)
                return run(*a, **k)

            slam.filterx.prefetch_launch = held_launch
            slam.run = run_after_junk
            slam.run_buffered(frames, intr, lookahead=lookahead, pipeline=True)
        torch.cuda.synchronize()
        k = slam.tracker.t1
        out.append((k, slam.keyframes.counter.value, slam.keyframes.tstamp[:slam.keyframes.counter.value].clone(), slam.keyframes.pose[:k].clone(),
                    slam.keyframes.depth[:k].clone(), slam.graph.edges_numpy(), slam.keyframes.featI[:slam.keyframes.counter.value].clone()))
    a, b = out
    print(f"[lookahead-streams] driver: {seen['launches']} launches held back, {seen['gathers']} gather chunks (still pending at the junk fill: {seen['pending']}), junk overlapped the batch {seen['overlaps']} times; "
          f"keyframes {a[1]} / {b[1]}, tracked {a[0]} / {b[0]}, poses equal {a[3].shape == b[3].shape and torch.equal(a[3], b[3])}, "
          f"depths equal {a[4].shape == b[4].shape and torch.equal(a[4], b[4])}, stored features equal {a[6].shape == b[6].shape and torch.equal(a[6], b[6])}")
    assert seen["launches"] == 4 and seen["gathers"] == 1 and len(seen["junk"]) == 1, seen
    assert seen["pending"] == 1, "the gather chunk's pass finished before the main stream drained: the delay was too short to decide the race"
    assert seen["overlaps"] == 0, "the gathered chunk's block went to the next main-stream allocation while its pass was held back"
    assert a[0] == b[0] and a[1] == b[1] and a[1] >= 8, (a[0], b[0], a[1], b[1])
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
    for x, y in zip(a[5], b[5]):
        np.testing.assert_array_equal(x, y)
    assert torch.equal(a[6], b[6]), "stored encoder features of the keyframes differ (the last two come from the gather chunk)"
