from .aligner import AlignmentExtractor, word_timestamps
from .generator import BannedSequenceProcessor, NGramRepeatBlockProcessor, SequenceGeneratorOptions
from .pretssel_generator import PretsselGenerator
from .prosody_encoder import ProsodyEncoder
from .transcriber import Transcriber, Transcription, TranscriptionToken, TranscriptionTokenStats
from .unit_extractor import UnitExtractor
from .translator import BatchedSpeechOutput, Modality, Task, Translator

__all__ = ["AlignmentExtractor", "BannedSequenceProcessor", "BatchedSpeechOutput", "Modality", "NGramRepeatBlockProcessor", "PretsselGenerator", "ProsodyEncoder", "SequenceGeneratorOptions", "Task", "Transcriber", "Transcription", "TranscriptionToken",
           "TranscriptionTokenStats", "Translator", "UnitExtractor", "word_timestamps"]
