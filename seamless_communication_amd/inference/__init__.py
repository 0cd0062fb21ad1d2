from .aligner import AlignmentExtractor, word_timestamps
from .generator import BannedSequenceProcessor, NGramRepeatBlockProcessor, PhraseBoostProcessor, SequenceGeneratorOptions, TopKSampler, TopPSampler
from .pretssel_generator import PretsselGenerator
from .prosody_encoder import ProsodyEncoder
from .transcriber import Transcriber, Transcription, TranscriptionToken, TranscriptionTokenStats
from .unit_extractor import UnitExtractor
from .translator import BatchedSpeechOutput, BeamHypothesis, LanguageId, MBRHypothesis, Modality, SampledHypothesis, Task, Translator

__all__ = ["AlignmentExtractor", "BannedSequenceProcessor", "BatchedSpeechOutput", "BeamHypothesis", "LanguageId", "MBRHypothesis", "Modality", "NGramRepeatBlockProcessor", "PhraseBoostProcessor", "PretsselGenerator", "ProsodyEncoder", "SampledHypothesis", "SequenceGeneratorOptions", "Task", "TopKSampler", "TopPSampler", "Transcriber", "Transcription", "TranscriptionToken",
           "TranscriptionTokenStats", "Translator", "UnitExtractor", "word_timestamps"]
