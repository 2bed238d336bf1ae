"""wenet_amd: MI355X-native Conformer-ASR inference path behind WeNet's API.

Public surface mirrors the reference (wenet/__init__.py:1, wenet/cli/model.py):
``load_model``, plus the search free functions, ``DecodeResult`` and the forced
alignment of ``ctc_utils.force_align`` (``wenet_amd.align``).
The compute path is hand-written HIP for gfx950 in ``libwenet_amd.so`` (C-ABI in
include/wenet_amd.h); it is loaded lazily and there is NO CPU fallback: using a
model without the library raises.
"""
__all__ = ["load_model", "ASRModel", "Transducer", "FireRed", "Branchformer", "Squeezeformer", "EfficientConformer", "Paraformer", "SenseVoiceSmall", "DecodeResult", "StreamingRecognizer",
           "RnntBeamStreamingRecognizer", "CtcEndpointConfig", "CtcEndpointRule", "AlignResult", "force_align",
           "force_align_batch"]


def __getattr__(name):
    if name in ("load_model", "ASRModel"):
        from wenet_amd import model as _m
        return getattr(_m, name)
    if name == "Transducer":
        from wenet_amd.transducer import Transducer
        return Transducer
    if name == "FireRed":
        from wenet_amd.firered import FireRed
        return FireRed
    if name == "Branchformer":
        from wenet_amd.branchformer import Branchformer
        return Branchformer
    if name == "Paraformer":
        from wenet_amd.paraformer import Paraformer
        return Paraformer
    if name == "SenseVoiceSmall":
        from wenet_amd.sensevoice import SenseVoiceSmall
        return SenseVoiceSmall
    if name == "Squeezeformer":
        from wenet_amd.squeezeformer import Squeezeformer
        return Squeezeformer
    if name == "EfficientConformer":
        from wenet_amd.efficonformer import EfficientConformer
        return EfficientConformer
    if name == "DecodeResult":
        from wenet_amd.search import DecodeResult
        return DecodeResult
    if name in ("StreamingRecognizer", "RnntBeamStreamingRecognizer", "CtcEndpointConfig",
                "CtcEndpointRule"):
        from wenet_amd import streaming as _s
        return getattr(_s, name)
    if name in ("AlignResult", "force_align", "force_align_batch"):
        from wenet_amd import align as _a
        return getattr(_a, name)
    raise AttributeError(name)
