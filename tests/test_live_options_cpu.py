"""CPU: which spec of harvest=, associate= and score= goes with time= on the two live predictors -- every pairing of a
spec with time= given or not, refused word for word or let through to the device lookup -- and which refusal a call with
several faults gets: the first option's in the order harvest, associate, score, ahead of any refusal of a size."""
import pytest

HARVEST_TIME = ("harvest= together with time= is not supported: a timed push is not one frame of a "
                "window (DESIGN.md 8)")
HARVEST_NEEDS = ("harvest=TimedHarvestSpec(...) needs time=TimeRule(...): its frames are instants of the "
                 "step grid (without time= the push-indexed HarvestSpec serves)")
ASSOC_NEEDS = ("associate=%s(...) needs time=TimeRule(...): its tracks are aged by time "
               "(without time= the push-indexed AssociateSpec serves)")
ASSOC_TIME = ("associate= together with time= is not supported: a velocity per tick and a gate that "
              "grows with the gap are a change of their own (DESIGN.md 8)")
SCORE_TIME = ("time= together with score= is not supported: the score records are indexed by push, and "
              "re-indexing them by time is a change of its own (DESIGN.md 8); the records indexed by "
              "time are score=TimedScoreSpec(...) (DESIGN.md 5.25)")
SCORE_NEEDS = ("score=TimedScoreSpec(...) needs time=TimeRule(...): its records are indexed by time "
               "(without time= the push-indexed ScoreSpec serves)")


def _model():
    from social_stgcnn_amd.model import social_stgcnn
    return social_stgcnn(n_stgcnn=1, n_txpcnn=5, output_feat=5, seq_len=8, kernel_size=3, pred_seq_len=12)


def _specs():
    """name -> (option, spec, the refusal when time= is given, the refusal when it is not); None: the pairing is right"""
    from social_stgcnn_amd import frames
    from social_stgcnn_amd.predict import ScoreSpec, TimedScoreSpec
    return {"HarvestSpec": ("harvest", frames.HarvestSpec(8), HARVEST_TIME, None),
            "TimedHarvestSpec": ("harvest", frames.TimedHarvestSpec(8), None, HARVEST_NEEDS),
            "AssociateSpec": ("associate", frames.AssociateSpec(1.0), ASSOC_TIME, None),
            "TimedAssociateSpec": ("associate", frames.TimedAssociateSpec(1.0), None, ASSOC_NEEDS % "TimedAssociateSpec"),
            "FilteredAssociateSpec": ("associate", frames.FilteredAssociateSpec(0.05, 1.0), None,
                                      ASSOC_NEEDS % "FilteredAssociateSpec"),
            "ScoreSpec": ("score", ScoreSpec(), SCORE_TIME, None),
            "TimedScoreSpec": ("score", TimedScoreSpec(), None, SCORE_NEEDS)}


SPECS = ("HarvestSpec", "TimedHarvestSpec", "AssociateSpec", "TimedAssociateSpec", "FilteredAssociateSpec", "ScoreSpec",
         "TimedScoreSpec")
# two faults in one call: the options by spec name, time= given or not, one more bad argument, and the refusal it gets
SEVERAL = [(("HarvestSpec", "AssociateSpec"), True, {}, HARVEST_TIME),
           (("TimedHarvestSpec", "TimedScoreSpec"), False, {}, HARVEST_NEEDS),
           (("FilteredAssociateSpec", "TimedScoreSpec"), False, {}, ASSOC_NEEDS % "FilteredAssociateSpec"),
           (("ScoreSpec",), True, dict(obs_len=0), SCORE_TIME),
           (("TimedAssociateSpec",), False, dict(capacity=0), ASSOC_NEEDS % "TimedAssociateSpec")]


def _make(cls, **kw):
    from social_stgcnn_amd import frames
    if cls == "FramePredictor":
        return frames.FramePredictor(_model(), **kw)
    return frames.StreamsPredictor(_model(), 3, **kw)


@pytest.mark.parametrize("timed", [True, False], ids=["time", "no_time"])
@pytest.mark.parametrize("spec", SPECS)
@pytest.mark.parametrize("cls", ["FramePredictor", "StreamsPredictor"])
def test_every_pairing_of_a_spec_with_time(cls, spec, timed):
    from social_stgcnn_amd.frames import TimeRule
    option, value, with_time, without_time = _specs()[spec]
    kw = {option: value, **(dict(time=TimeRule(10)) if timed else {})}
    refusal = with_time if timed else without_time
    if refusal is None:                                      # past every check: the device lookup ends it on this machine
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            _make(cls, **kw)
        return
    with pytest.raises(ValueError) as e:
        _make(cls, **kw)
    assert str(e.value) == refusal


@pytest.mark.parametrize("names,timed,more,refusal", SEVERAL, ids=[",".join(c[0] + tuple(c[2])) for c in SEVERAL])
@pytest.mark.parametrize("cls", ["FramePredictor", "StreamsPredictor"])
def test_the_first_option_wrongly_paired_is_the_one_refused(cls, names, timed, more, refusal):
    from social_stgcnn_amd.frames import TimeRule
    specs = _specs()
    kw = {specs[n][0]: specs[n][1] for n in names}
    with pytest.raises(ValueError) as e:
        _make(cls, **kw, **more, **(dict(time=TimeRule(10)) if timed else {}))
    assert str(e.value) == refusal
