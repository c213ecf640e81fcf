"""Keywords in wav files of any length and sample rate, one line per detection:
python scripts/spot_wav.py MODEL_TYPE CHECKPOINT WANTED_WORDS WAV [WAV ...] [--representation mfcc] [--hop 320] ...

MODEL_TYPE is a model of model.speech_model, CHECKPOINT what Model.save_weights / Model.save wrote, WANTED_WORDS the
comma-separated words the model was trained on (the classes are input_data.prepare_words_list of them: _silence_, _unknown_,
then the words).  --representation names what the model takes, as AudioProcessor's output_representation did in training:
'raw' (the default: the windows themselves) or the STFT features 'mfcc', 'spec', 'mfcc_and_raw' with the framing of
--window-ms / --stride-ms / --dct-coefficient-count / --num-log-mel-features (defaults: 30 ms / 10 ms, 40 / 40, what
conv_1d_log_mfcc takes).  The feature models' overlapping windows share their STFT frames (stream.Features.rows; the hop must
be a multiple of the frame step); --no-share-frames computes every window's own, for any hop."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speech_recognition_amd import input_data, stream  # noqa: E402
from speech_recognition_amd.model import prepare_model_settings, speech_model  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("model_type")
    ap.add_argument("checkpoint")
    ap.add_argument("wanted_words")
    ap.add_argument("wavs", nargs="+")
    ap.add_argument("--representation", choices=("raw", "mfcc", "spec", "mfcc_and_raw"), default="raw")
    ap.add_argument("--sample-rate", type=int, default=16000)
    ap.add_argument("--clip-ms", type=int, default=1000)
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--stride-ms", type=float, default=10.0)
    ap.add_argument("--dct-coefficient-count", type=int, default=40)
    ap.add_argument("--num-log-mel-features", type=int, default=40)
    ap.add_argument("--no-share-frames", action="store_true")
    ap.add_argument("--hop", type=int, default=320)
    ap.add_argument("--average-ms", type=int, default=500)
    ap.add_argument("--threshold", type=float, default=0.7)
    ap.add_argument("--suppression-ms", type=int, default=1000)
    ap.add_argument("--minimum-count", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--rate-policy", choices=input_data.RATE_POLICIES, default="resample")
    a = ap.parse_args()
    labels = input_data.prepare_words_list([w for w in a.wanted_words.split(",") if w])
    settings = prepare_model_settings(len(labels), a.sample_rate, a.clip_ms, a.window_ms, a.stride_ms, a.dct_coefficient_count,
                                      a.num_log_mel_features, output_representation=a.representation)
    extra = {}
    if a.representation == "raw":
        model = speech_model(a.model_type, settings['desired_samples'], len(labels))
    else:
        model = speech_model(a.model_type, settings['fingerprint_size'], num_classes=settings['label_count'], **settings)
        extra = dict(features=stream.Features(settings, output_representation=a.representation),
                     share_frames=not a.no_share_frames)
    model.load_weights(a.checkpoint)
    for wav in a.wavs:
        r = stream.spot_wav(model, wav, labels=labels, rate_policy=a.rate_policy, sample_rate=a.sample_rate, hop=a.hop,
                            average_ms=a.average_ms, threshold=a.threshold, suppression_ms=a.suppression_ms,
                            minimum_count=a.minimum_count, batch=a.batch, **extra)
        for label, time_s, sample, score in r.detections:
            print("%s\t%.3f s\tsample %d\t%s\t%.3f" % (wav, time_s, sample, label, score))
        print("%s: %d detections in %d windows" % (wav, len(r.detections), r.W), file=sys.stderr)


if __name__ == "__main__":
    main()
