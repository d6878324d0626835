"""The text side of the reference's asr_evaluation.py (:27-32): the transcripts are lower-cased, their punctuation is dropped (what jiwer's
RemovePunctuation and ToLowerCase do) and scored as words on the device.  The recogniser the reference runs first (DeepSpeech) and unidecode are
third-party and stay out: score_transcripts takes the recognised text.
"""
import logging
import unicodedata

from .recognition_model import word_errors


def normalize_transcript(text):
    """Lower case, every character of a Unicode punctuation category (P*) dropped."""
    return ''.join(c for c in text if not unicodedata.category(c).startswith('P')).lower()


def score_transcripts(targets, predictions, *, device=None):
    """ErrorCounts (hits, substitutions, deletions, insertions, reference words, WER, per-utterance results) of the predicted transcripts against
    the target transcripts after normalize_transcript, logged as the reference logs them."""
    targets, predictions = [normalize_transcript(t) for t in targets], [normalize_transcript(p) for p in predictions]
    if len(targets) != len(predictions):
        raise ValueError('score_transcripts: %d targets for %d predictions' % (len(targets), len(predictions)))
    counts = word_errors(targets, predictions, device=device)
    logging.info(f'targets: {targets}')
    logging.info(f'predictions: {predictions}')
    logging.info(f'wer: {counts.rate}')
    return counts
