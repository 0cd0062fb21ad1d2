"""Streaming S2ST / S2TT (BASELINE cfg 5): the reference's SimulEval agent chain on the HIP path."""
from .agents import (DetokenizerAgent, DualVocoderAgent, MMATextDecoderAgent, NARUnitYUnitDecoderAgent, OfflineWav2VecBertEncoderAgent, OnlineFeatureExtractorAgent,
                     PretsselVocoderAgent, SeamlessS2STAgent, SeamlessS2STDualVocoderAgent, SeamlessStreamingS2STAgent,
                     SeamlessStreamingS2TAgent, SeamlessStreamingS2TDetokAgent,
                     UnitYMMATextDecoderAgent, VocoderAgent, default_args)
from .backend import HipStreamingBackend
from .pool import HipPoolBackend, SerialPoolBackend, StreamingSessionPool
from .vad import (SeamlessS2STDualVocoderVADAgent, SeamlessS2STVADAgent, SeamlessStreamingS2STVADAgent, SeamlessStreamingS2TVADAgent,
                  SpeechVADAgent, SpeechVADStates, VADStream, vad_args)
from .simul import EmptySegment, ReadAction, Segment, SpeechSegment, TextSegment, WriteAction

__all__ = [
    "DetokenizerAgent", "DualVocoderAgent", "EmptySegment", "HipPoolBackend", "HipStreamingBackend", "MMATextDecoderAgent", "NARUnitYUnitDecoderAgent", "OfflineWav2VecBertEncoderAgent",
    "OnlineFeatureExtractorAgent", "PretsselVocoderAgent", "ReadAction", "SeamlessS2STAgent", "SeamlessS2STDualVocoderAgent", "SeamlessStreamingS2STAgent", "SeamlessStreamingS2TAgent", "SeamlessStreamingS2TDetokAgent", "Segment",
    "SerialPoolBackend", "SpeechSegment", "StreamingSessionPool", "TextSegment", "UnitYMMATextDecoderAgent", "VocoderAgent", "WriteAction", "default_args",
    "SeamlessS2STDualVocoderVADAgent", "SeamlessS2STVADAgent", "SeamlessStreamingS2STVADAgent", "SeamlessStreamingS2TVADAgent", "SpeechVADAgent",
    "SpeechVADStates", "VADStream", "vad_args",
]
