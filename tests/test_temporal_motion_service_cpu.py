"""CPU: the noise-map keyword of both services and both nodes - ``HipUpscalerService(denoise_temporal=True, noise_map='motion')`` and
``HipEgvsrUpscalerService(denoise_temporal=True, denoise_noise_map='motion')`` - pure Python, no GPU, no process.  Checked: the words that are
accepted, ``ValueError`` for any other word and for ``'motion'`` without ``denoise_temporal`` (the per-frame denoiser keeps no previous input
frame on the device), that the keyword reaches the binding's constructor - and that the default builds the object with the arguments it was
built with before the keyword existed -, that ``TemporalNode`` / ``TemporalEgvsrNode`` hand the keyword to their workers, and that ``EgvsrNode``
keeps refusing the temporal keywords."""
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd.egvsr_node import EgvsrNode
from sharkshark4k_amd.temporal_node import TemporalEgvsrNode, TemporalNode
from sharkshark4k_amd.upscale.egvsr_upscaler import HipEgvsrUpscalerService
from sharkshark4k_amd.upscale.hip_upscaler import HipUpscalerService, validate_noise_map
from tests.frvsr_temporal_node_double import DoubleFrvsrTemporalService
from tests.temporal_node_double import DoubleTemporalService

BAD_WORDS = ["Motion", "adaptive", "", None, 1, True, b"motion", ("motion",)]


def fsrcnn(**kw):
    return HipUpscalerService(denoising=True, upscaler_model="fsrcnn", lr_shape=(16, 24), weights="synthetic", **kw)


def egvsr(**kw):
    return HipEgvsrUpscalerService(**dict(dict(lr_shape=(16, 24), weights="synthetic"), **kw))


def test_the_words_and_where_they_belong():
    assert validate_noise_map("constant", False) == "constant" and validate_noise_map("motion", True) == "motion"
    assert _capi.noise_map_mode("constant") == 0 and _capi.noise_map_mode("motion") == 1 and _capi.NOISE_MAPS == {"constant": 0, "motion": 1}
    for word in BAD_WORDS:
        with pytest.raises(ValueError, match="noise"):
            _capi.noise_map_mode(word)
    # the per-frame service
    assert fsrcnn().noise_map == "constant" and fsrcnn(noise_map="constant").noise_map == "constant"
    assert fsrcnn(denoise_temporal=True).noise_map == "constant"
    assert fsrcnn(denoise_temporal=True, noise_map="motion", max_streams=3).noise_map == "motion"
    with pytest.raises(ValueError, match=r"noise_map='motion' belongs to denoise_temporal=True"):
        fsrcnn(noise_map="motion")
    with pytest.raises(ValueError, match=r"noise_map='motion' belongs to denoise_temporal=True"):
        fsrcnn(noise_map="motion", denoise_temporal=False)
    for word in BAD_WORDS:
        for temporal in (False, True):
            with pytest.raises(ValueError, match="noise_map="):
                fsrcnn(noise_map=word, denoise_temporal=temporal)
    # the frame-recurrent service
    assert egvsr().denoise_noise_map == "constant" and egvsr(denoise_temporal=True).denoise_noise_map == "constant"
    assert egvsr(denoise_temporal=True, denoise_noise_map="motion", denoise_pad=True, lr_shape=(15, 17)).denoise_noise_map == "motion"
    with pytest.raises(ValueError, match=r"denoise_noise_map='motion' belongs to denoise_temporal=True"):
        egvsr(denoise_noise_map="motion")
    for word in BAD_WORDS:
        for temporal in (False, True):
            with pytest.raises(ValueError, match="denoise_noise_map="):
                egvsr(denoise_noise_map=word, denoise_temporal=temporal)
    assert not torch.cuda.is_initialized()


class Recorded:
    """Stands where the binding's object would be made and keeps what it was made with."""
    made = []

    def __init__(self, *args, **kw):
        Recorded.made.append((args, kw))

    def stream_state_bytes_for(self):
        return 1 << 20


def test_the_keyword_reaches_the_bindings_constructor(monkeypatch):
    monkeypatch.setattr(_capi, "TemporalUpscaler", Recorded)
    monkeypatch.setattr(_capi, "TemporalFrvsrUpscaler", Recorded)
    for kw, want in (({}, None), ({"noise_map": "constant"}, None), ({"noise_map": "motion"}, "motion"), ({"noise_map": "motion", "max_streams": 3}, "motion")):
        svc = fsrcnn(denoise_temporal=True, **kw)
        svc.output_shape = None
        js = {"up": None, "key": None, "ctx": "ctx", "model": "sr", "denoise": "dn"}
        svc._job_set = lambda k, js=js: js
        Recorded.made.clear()
        up = svc._get_upscaler(0)
        assert isinstance(up, Recorded) and len(Recorded.made) == 1
        args, made_kw = Recorded.made[0]
        assert made_kw.get("noise_map") == want and ("noise_map" in made_kw) == (want is not None)   # constant: built as before the keyword
        assert made_kw.get("max_streams", 1) == kw.get("max_streams", 1) and args[:3] == ("ctx", "sr", "dn")
    for kw, want in (({}, None), ({"denoise_noise_map": "constant"}, None), ({"denoise_noise_map": "motion"}, "motion"),
                     ({"denoise_noise_map": "motion", "denoise_pad": True, "denoise_scene_cut": 12.0}, "motion")):
        svc = egvsr(denoise_temporal=True, **kw)
        svc.ctx, svc.model, svc.denoise_model = "ctx", "m", "dn"
        Recorded.made.clear()
        up = svc._make_upscaler(_capi, ((16, 24), None))
        assert isinstance(up, Recorded) and len(Recorded.made) == 1
        args, made_kw = Recorded.made[0]
        assert made_kw.get("noise_map") == want and ("noise_map" in made_kw) == (want is not None)
        assert made_kw.get("pad", False) == kw.get("denoise_pad", False) and made_kw.get("scene_cut") == kw.get("denoise_scene_cut")
        assert "denoise_noise_map" not in made_kw


class NodeDouble(DoubleTemporalService):
    def __init__(self, *a, noise_map="constant", **kw):
        super().__init__(*a, **kw)
        self.noise_map = noise_map


class EgvsrNodeDouble(DoubleFrvsrTemporalService):
    def __init__(self, *a, denoise_noise_map="constant", **kw):
        super().__init__(*a, **kw)
        self.denoise_noise_map = denoise_noise_map


def test_both_nodes_pass_the_keyword_to_their_workers():
    common = dict(devices=[10, 11], max_streams=2, job_frames=4, ends_per_part=1, host_frames=(3, 4), host_slots=3, push_timeout=5.0, lr_shape=(3, 4))
    for cls, double, key, words in ((TemporalNode, NodeDouble, "noise_map", ("motion", "constant")),
                                    (TemporalEgvsrNode, EgvsrNodeDouble, "denoise_noise_map", ("motion", "constant"))):
        for word in words:
            n = cls(service_cls=double, **dict(common, **{key: word}))
            try:
                assert len(n.services) == 2 and all(getattr(svc, key) == word for svc in n.services)
            finally:
                n.close()
        n = cls(service_cls=double, **common)                       # not given: the worker's own default
        try:
            assert all(getattr(svc, key) == "constant" for svc in n.services)
        finally:
            n.close()
    # the real services in the node's process (no worker is started): the word arrives and is validated there
    n = TemporalEgvsrNode(devices=[0], job_frames=2, host_frames=(20, 30), host_slots=2, output_shape=None, lr_shape=(13, 22), weights="synthetic",
                          denoise_pad=True, denoise_noise_map="motion")
    try:
        assert type(n.services[0]) is HipEgvsrUpscalerService and n.services[0].denoise_noise_map == "motion" and n.services[0].denoise_temporal
    finally:
        n.close()
    with pytest.raises(ValueError, match="denoise_noise_map="):
        TemporalEgvsrNode(devices=[0], job_frames=2, host_frames=(20, 30), host_slots=2, output_shape=None, lr_shape=(16, 24), weights="synthetic",
                          denoise_noise_map="fast")
    n = TemporalNode(devices=[0], job_frames=2, host_frames=(20, 30), host_slots=2, output_shape=None, lr_shape=(16, 24), weights="synthetic",
                     denoising=True, upscaler_model="fsrcnn", noise_map="motion")
    try:
        assert type(n.services[0]) is HipUpscalerService and n.services[0].noise_map == "motion" and n.services[0].denoise_temporal
    finally:
        n.close()
    with pytest.raises(ValueError, match="noise_map="):
        TemporalNode(devices=[0], job_frames=2, host_frames=(20, 30), host_slots=2, output_shape=None, lr_shape=(16, 24), weights="synthetic",
                     denoising=True, upscaler_model="fsrcnn", noise_map="fast")
    assert not torch.cuda.is_initialized()


def test_egvsr_node_keeps_refusing_the_temporal_keywords():
    args = dict(devices=[0], host_frames=(16, 24), host_slots=2, output_shape=None, lr_shape=(16, 24), weights="synthetic")
    with pytest.raises(ValueError, match=r"EgvsrNode\(denoise_temporal=True\)"):
        EgvsrNode(denoise_temporal=True, denoise_noise_map="motion", **args)
    with pytest.raises(ValueError, match=r"denoise_noise_map='motion' belongs to denoise_temporal=True"):
        EgvsrNode(denoise_noise_map="motion", **args)               # without the denoiser the service itself refuses the word
