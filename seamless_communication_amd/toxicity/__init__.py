"""MinTox: mitigation of added toxicity at inference time (reference ``seamless_communication.toxicity``): the ETOX
word-list checker and the re-decode pipeline whose banned-sequence step processor runs inside the HIP beam-search step."""
from .etox_bad_word_checker import ETOXBadWordChecker, load_etox_bad_word_checker
from .mintox import mintox_pipeline

__all__ = ["ETOXBadWordChecker", "load_etox_bad_word_checker", "mintox_pipeline"]
