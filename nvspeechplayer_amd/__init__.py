"""nvspeechplayer_amd -- MI355X-native Klatt synthesis engine behind the speechPlayer C-ABI."""
from . import _native  # noqa: F401
from .speechPlayer import BatchPlayer, Frame, LiveGroup, NodePlayer, SpeechPlayer, frameResponse, host_array, melFilterbank, MixTerm, mixTermDtype, pcmConvolve, pcmMix, pcmResample, pcmSpectrogram, resampleKernel, resonatorCoefficients, setGlobalOption, check_signal_request, signalConvolve, signalMix, signalPower, signalResample, signalSpectrogram  # noqa: F401

__all__ = ["Frame", "SpeechPlayer", "BatchPlayer", "NodePlayer", "LiveGroup", "host_array", "setGlobalOption", "frameResponse", "resonatorCoefficients", "pcmSpectrogram", "melFilterbank", "pcmResample", "resampleKernel", "pcmConvolve", "pcmMix", "MixTerm", "mixTermDtype", "signalSpectrogram", "signalResample", "signalConvolve", "signalMix", "signalPower", "check_signal_request"]
