"""FusionFramePipeline without a GPU: the hysteresis / auto-switch class against a literal
transcription of fused_depth_map.py:2515-2571, and the argument validation of the pipeline."""
import os

import numpy as np
import pytest

os.environ.setdefault("SV_WARMUP_AT_IMPORT", "0")
from frame_chain import LoopTranscription  # noqa: E402  (the literal transcription of :2515-2571)
from stereovision_amd.frame import OUTPUT_NAMES, FusionFramePipeline, OcclusionSwitch  # noqa: E402


def _drive(script, toggles=()):
    """script: the detector's answer for every frame; toggles: {frame index: use_stereo set by
    hand before that frame}.  Returns the switch's (state, use_stereo) after every frame, checked
    against the transcription on the way."""
    ref, sw = LoopTranscription(), OcclusionSwitch()
    toggles = dict(toggles)
    out, checks = [], 0
    for i, detected in enumerate(script):
        if i in toggles:
            ref.USE_STEREO = sw.use_stereo = toggles[i]
        ref.frame(detected)
        if sw.due():
            checks += 1
            sw.update(detected)
        sw.tick()
        assert (sw.state, sw.use_stereo) == (ref.occlusion_state, ref.USE_STEREO), i
        assert sw.frame_counter == ref.frame_counter
        out.append((sw.state, sw.use_stereo))
    assert checks == ref.checked
    return out


def test_hysteresis_and_auto_switch(capsys):
    # only every second frame is checked: answers on odd frames are never seen
    out = _drive(['none', 'left'] * 10)
    assert all(s == ('none', True) for s in out)
    sw = OcclusionSwitch()
    seen = []
    for i in range(6):
        seen.append(sw.due())
        sw.tick()
    assert seen == [True, False, True, False, True, False]      # a pipeline's first frame is checked

    # a flicker shorter than 5 checks never switches (4 disagreeing checks, then agreement resets)
    out = _drive((['left'] * 8 + ['none'] * 2) * 3)
    assert all(s == ('none', True) for s in out)

    # exactly 5 consecutive disagreeing checks switch: checks fall on frames 0, 2, 4, 6, 8
    out = _drive(['left'] * 12)
    assert out[7] == ('none', True) and out[8] == ('left', False)
    assert all(s == ('left', False) for s in out[8:])

    # 'right' switches stereo off as well; 'both' switches it back on, and so does 'none'
    out = _drive(['right'] * 10 + ['both'] * 10 + ['left'] * 10 + ['none'] * 10)
    assert out[8] == ('right', False) and out[17] == ('right', False) and out[18] == ('both', True)
    assert out[28] == ('left', False) and out[38] == ('none', True)

    # a manual toggle holds until the next confirmed change, which overrides it
    out = _drive(['none'] * 4 + ['left'] * 12 + ['none'] * 12, toggles={1: False, 20: True})
    assert out[1] == ('none', False) and out[11] == ('none', False)         # stays off: no change confirmed
    assert out[12] == ('left', False)                                         # confirmed 'left': already off
    assert out[20] == ('left', True)                                          # switched on by hand while covered
    assert out[23] == ('left', True) and out[24] == ('none', True)          # 'none' confirmed: stays on
    out = _drive(['left'] * 12, toggles={3: False, 5: True})
    assert out[5] == ('none', True) and out[8] == ('left', False)           # the toggle is overridden

    # other intervals and thresholds
    sw = OcclusionSwitch(check_interval=1, hysteresis_frames=2)
    states = []
    for d in ['left', 'none', 'left', 'left', 'both', 'both']:
        if sw.due():
            sw.update(d)
        sw.tick()
        states.append((sw.state, sw.use_stereo))
    assert states == [('none', True), ('none', True), ('none', True), ('left', False), ('left', False),
                      ('both', True)]
    capsys.readouterr()


def test_argument_validation():
    with pytest.raises(ValueError, match="unknown outputs"):
        FusionFramePipeline(outputs=("fused_u8", "fused_depth"))
    with pytest.raises(ValueError):
        FusionFramePipeline(occlusion_check_interval=0)
    for name in OUTPUT_NAMES:
        FusionFramePipeline(outputs=(name,))
    pipe = FusionFramePipeline(outputs=())
    bgr = np.zeros((60, 80, 3), np.uint8)
    # a non-uint8 frame, a frame that is no array, a frame of another rank, a pair of two sizes:
    # raised by step before any engine is needed
    with pytest.raises(TypeError, match="frame_right: uint8"):
        pipe.step(bgr, bgr.astype(np.float32))
    with pytest.raises(TypeError, match="frame_left"):
        pipe.step(None, bgr)
    with pytest.raises(ValueError, match="frame_left"):
        pipe.step(bgr[..., 0], bgr)
    with pytest.raises(ValueError, match="differ in shape"):
        pipe.step(bgr, bgr[:50])
    with pytest.raises(TypeError, match="midas_raw"):
        pipe.step(bgr, bgr, midas=np.zeros((60, 80), np.float64))
    with pytest.raises(ValueError, match="midas_raw"):
        pipe.step(bgr, bgr, midas=(np.zeros((60, 80, 1), np.float32), None))
    with pytest.raises(TypeError, match="midas_conf"):
        pipe.step(bgr, bgr, midas=(np.zeros((60, 80), np.float32), np.zeros((60, 80), np.uint8)))
    assert pipe.frame_counter == 0                                # a refused step is no frame
    # a MiDaS map of another size is legal: the reference resizes it (fused_depth_map.py:1215)
    small = np.ones((40, 50), np.float32)
    left, right, raw = FusionFramePipeline.check_inputs(bgr, bgr, small)
    assert raw.shape == (40, 50) and left.shape == right.shape == (60, 80, 3)
    assert FusionFramePipeline.check_inputs(bgr, bgr, (small, small))[2].shape == (40, 50)
    assert FusionFramePipeline.check_inputs(bgr, bgr, (None, None))[2] is None
    assert FusionFramePipeline.check_inputs(bgr, bgr)[2] is None
    # the result's map lookup knows the same names
    from stereovision_amd.frame import FrameResult
    r = FrameResult()
    assert r.device("fused_u8") is None and r.fused_u8 is None and r.mode_text is None
    with pytest.raises(ValueError):
        r.device("fused_depth")
