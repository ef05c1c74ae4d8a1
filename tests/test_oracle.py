"""CPU: the oracle against the golden vectors captured from the reference
(tests/golden/generate.py), and the known answers of SURVEY.md App. E."""
import math

import numpy as np
import pytest
import torch

from conftest import case_inputs, case_names, seconds, variant_config, \
    variant_state
from emphases_amd import synth, weights
from oracle import librosa_mel
from oracle import prominence as oracle

CASES = ['two_tone_1s', 'utt_2p5s', 'utt_10s', 'utt_silence_6s',
         'short_words_3s', 'float_floor_17s', 'chunked_41s_b500',
         'chunked_41s_b1000']


@pytest.fixture(scope='module')
def state():
    return {k: torch.from_numpy(v) for k, v in weights.load().items()}


def test_case_list_is_complete(cases):
    assert case_names(cases) == sorted(CASES)


@pytest.mark.parametrize('name', CASES)
def test_scores_match_reference(cases, state, name):
    audio, bounds, batch_size = case_inputs(cases, name)
    scores = oracle.from_alignment_and_audio(
        seconds(bounds), torch.from_numpy(audio), state, {}, batch_size)
    assert scores.dtype == torch.float32
    np.testing.assert_allclose(
        scores[0].numpy(), cases[f'{name}/scores'], rtol=0, atol=2e-6)
    # the shipped bf16 autocast path is only informational: ~2e-3 away
    shipped = cases[f'{name}/scores_shipped_bf16']
    assert np.abs(shipped - cases[f'{name}/scores']).max() < 5e-3


@pytest.mark.parametrize('name', ['two_tone_1s', 'utt_2p5s', 'short_words_3s'])
def test_stages_match_reference(cases, state, name):
    audio, bounds, _ = case_inputs(cases, name)
    padded = torch.nn.functional.pad(torch.from_numpy(audio), (432, 432))
    mel = oracle.logmel(padded[:, :audio.shape[1]])
    np.testing.assert_allclose(
        mel.numpy(), cases[f'{name}/mel'], rtol=0, atol=1e-5)
    stages = {}
    oracle.forward(mel, bounds, state, {}, stages)
    for key in ('input_layer', 'encoder', 'downsampled', 'logits'):
        np.testing.assert_allclose(
            stages[key].numpy(), cases[f'{name}/{key}'], rtol=0, atol=2e-5,
            err_msg=key)


def test_known_answers_of_the_survey(cases):
    """1 s two-tone signal, bundled checkpoint, fp32."""
    mel = cases['two_tone_1s/mel']
    np.testing.assert_allclose(
        mel[:4, 0], [-4.0047779, -3.8994355, -3.6789193, -3.4502010],
        atol=2e-6)
    np.testing.assert_allclose(
        mel[:4, 50], [-9.0457182, -8.5435104, -7.6494780, -6.2575841],
        atol=2e-5)
    np.testing.assert_allclose(
        cases['two_tone_1s/logits'],
        [-1.2813212, -1.3857896, -1.1205515, -2.7076979], atol=2e-6)
    np.testing.assert_allclose(
        cases['two_tone_1s/scores'],
        [0.2173254, 0.2000808, 0.2459090, 0.0625206], atol=1e-6)
    np.testing.assert_allclose(
        cases['two_tone_1s/scores_shipped_bf16'],
        [0.2158203, 0.2001953, 0.2460938, 0.0629883], atol=1e-6)


def test_mel_basis_known_answers():
    basis = librosa_mel.mel(sr=16000, n_fft=1024, n_mels=80)
    assert basis.shape == (80, 513) and basis.dtype == np.float32
    assert np.count_nonzero(basis) == 1001
    assert np.all(basis[:, 512] == 0)
    counts = (basis != 0).sum(1)
    assert counts.min() == 4 and counts.max() == 37
    assert 0.0622 < basis.sum(1).min() and basis.sum(1).max() < 0.0666
    # the one external anchor: the value printed in librosa's documentation
    doc = librosa_mel.mel(sr=22050, n_fft=2048, n_mels=128)
    assert abs(float(doc[0, 1]) - 0.016182853) < 1e-9


def test_loudness_known_answers():
    """SURVEY.md App. E loudness row of the two-tone signal."""
    n = np.arange(16000, dtype=np.float64)
    x = 0.1 * np.sin(2 * np.pi * 220 * n / 16000) + \
        0.05 * np.sin(2 * np.pi * 1000 * n / 16000)
    audio = torch.from_numpy(x.astype(np.float32))[None]
    chunk = torch.nn.functional.pad(audio, (432, 432))[:, :16000]
    loud = oracle.loudness(chunk)[0].numpy()
    np.testing.assert_allclose(
        loud[0:3], [-64.263748, -55.540615, -52.383636], atol=2e-4)
    np.testing.assert_allclose(
        loud[50:53], [-71.353615, -71.353981, -71.355431], atol=2e-4)
    assert abs(loud.mean() + 70.118088) < 2e-4
    silent = oracle.loudness(torch.zeros(1, 16000))[0].numpy()
    assert np.all(silent == -100.0)
    weights_ = oracle.a_weights()[:, 0]
    np.testing.assert_allclose(
        weights_[[0, 1, 2, 128, 512]],
        [-100.0, -98.32126992, -77.08839866, -19.99965554, -19.03635464],
        atol=1e-6)


def test_variant_matrix_matches_reference(variants):
    """Every config variant of SURVEY.md App. A.6 with seeded weights."""
    audio = torch.from_numpy(synth.pcm_to_float(variants['audio_pcm']))
    bounds = variants['bounds_frames'].astype(np.int64)
    padded = torch.nn.functional.pad(audio, (432, 432))
    checked = 0
    for name in variants['names']:
        config, overrides = variant_config(name)
        state = {k: torch.from_numpy(v) for k, v in
                 variant_state(variants, name, config).items()}
        feats = oracle.features(
            padded[:, :audio.shape[1]], overrides, synth.pitch_tracks)[0]
        logits = oracle.forward(feats, bounds, state, overrides).numpy()
        want = variants[f'{name}/logits']
        scale = float(np.abs(want).max())
        assert 2. < scale <= 4., (name, scale)        # (the goldens' output gain)
        assert np.abs(logits - want).max() < 5e-6 * scale, name
        scores = oracle.postprocess(torch.from_numpy(logits), config.loss)
        assert np.abs(scores.numpy() -
                      variants[f'{name}/scores']).max() < 2e-6, name
        if config.loudness_feature or config.pitch_feature or \
                config.periodicity_feature:
            np.testing.assert_allclose(
                feats.numpy(), variants[f'{name}/features'][0]
                if variants[f'{name}/features'].ndim == 3
                else variants[f'{name}/features'], atol=2e-4)
        checked += 1
    assert checked == len(variants["names"]) == 39


def test_metrics_restatement_known_answers():
    """oracle/metrics.py (emphases/evaluate/metrics.py:12-110) on values that
    can be checked by hand."""
    from oracle import metrics
    logits = torch.tensor([[[0., 2., -1.]], [[1., 9., 9.]]])
    targets = torch.tensor([[[0.5, 1., 0.]], [[0., 7., 7.]]])
    lengths = torch.tensor([3, 1])
    m = metrics.Metrics((0.5, 0.25), (0.25, 0.5), 'bce')
    m.update(logits, targets, lengths)
    p = torch.sigmoid(torch.tensor([0., 2., -1., 1.]))
    t = torch.tensor([0.5, 1., 0., 0.])
    want_bce = float(-(t * torch.log(p) + (1 - t) * torch.log(1 - p)).mean())
    got = m()
    assert abs(got['bce'] - want_bce) < 1e-6
    assert abs(got['mse'] - float(((p - t) ** 2).mean())) < 1e-7
    want_r = float(((p - 0.5) * (t - 0.25)).sum()) / 4 / (0.25 * 0.5)
    assert abs(got['pearson_correlation'] - want_r) < 1e-6
    mean, std = metrics.mean_std([1., 2., 3., 4.])
    assert mean == 2.5 and abs(std - 1.2909944487358056) < 1e-12
    clamped = metrics.Metrics((0., 1.), (0., 1.), 'mse')
    clamped.update(torch.tensor([[[2., -3.]]]), torch.tensor([[[1., 0.]]]),
                   torch.tensor([2]))
    assert abs(clamped()['mse']) < 1e-12          # clamp(2)=1, clamp(-3)=0


###############################################################################
# resampling (torchaudio is third-party and absent: the
# restatement is anchored on closed-form answers)
###############################################################################


def windowed_sinc_gain(nu):
    """Continuous-time frequency response of sinc(u) hann(u), |u| < 6, at nu =
    f / (cut-off): the integral of sin(pi u)/(pi u) (1 + cos(pi u / 6))/2
    cos(pi nu u) du over [-6, 6], written with sine integrals."""
    from scipy.special import sici
    a = 6 * np.pi
    si = lambda x: sici(x)[0]        # noqa: E731
    return (si(a * (1 + nu)) + si(a * (1 - nu))) / (2 * np.pi) + (
        si(a * (1 + nu + 1 / 6)) + si(a * (1 + nu - 1 / 6)) +
        si(a * (1 - nu + 1 / 6)) + si(a * (1 - nu - 1 / 6))) / (4 * np.pi)


RATES = [8000, 22050, 44100, 48000]


@pytest.mark.parametrize('rate', RATES)
def test_resample_known_answers(rate):
    """oracle/resample.py: output lengths, DC gain and the amplitude / phase
    of a 1 kHz sinusoid against the closed-form response of the Hann-windowed
    sinc (zero phase: the filter is symmetric).  When upsampling, the image of
    DC at the input rate sits in the transition band and leaves a 4e-4 ripple
    (a property of the filter, not of the restatement)."""
    from oracle import resample as oracle_resample
    for length in (0, 1, 5, rate // 3 + 17, rate):
        got = oracle_resample.resample(np.zeros(length), rate)
        assert len(got) == -(-16000 * length // rate) == \
            oracle_resample.output_length(length, rate, 16000)
    count = rate // 2
    interior = slice(2000, 6000)             # of the 8000 output samples
    dc = oracle_resample.resample(np.ones(count), rate)[interior]
    ripple = {8000: 5e-4, 22050: 1e-4}.get(rate, 5e-6)
    assert np.abs(dc - windowed_sinc_gain(0.)).max() < ripple
    tone = np.sin(2 * np.pi * 1000. * np.arange(count) / rate)
    got = oracle_resample.resample(tone, rate)
    cutoff = min(rate, 16000) * 0.99 / 2
    want = windowed_sinc_gain(1000. / cutoff) * np.sin(
        2 * np.pi * 1000. * np.arange(len(got)) / 16000.)
    assert np.abs(got[interior] - want[interior]).max() < 1e-4
    assert abs(windowed_sinc_gain(1000. / cutoff) - 1) < 5e-4
    # an impulse comes back as the filter itself (peak base / orig at its time)
    impulse = np.zeros(64 * rate // math.gcd(rate, 16000))
    impulse[len(impulse) // 2] = 1.
    response = oracle_resample.resample(impulse, rate)
    orig, new = oracle_resample.reduced(rate, 16000)
    assert abs(response.max() - np.float32(min(orig, new) * 0.99 / orig)) < 1e-7
    assert response.argmax() == (len(impulse) // 2) * new // orig


@pytest.mark.parametrize('rate', RATES)
def test_resample_table_matches_oracle(rate):
    """The product's polyphase TABLE (`emphases_amd.load.resample_kernel`,
    built on the host like every weight pack; `emph_resample` applies it on
    the device) against the independent restatement: the table is applied
    here, in the test, as the strided correlation it describes."""
    from emphases_amd import load
    from oracle import resample as oracle_resample
    kernel, orig, new, width = load.resample_kernel(rate)
    taps = kernel.reshape(new, -1).numpy().astype(np.float64)
    for index, length in enumerate((rate // 3 + 17, 5, 1)):
        audio = synth.weights(200 + index, (length,), 0.9)
        padded = np.concatenate(
            [np.zeros(width), audio.astype(np.float64),
             np.zeros(width + orig)])
        steps = (len(padded) - taps.shape[1]) // orig + 1
        windows = np.lib.stride_tricks.sliding_window_view(
            padded, taps.shape[1])[::orig][:steps]
        got = (windows @ taps.T).reshape(-1)[
            :load.resampled_length(length, orig, new)]
        want = oracle_resample.resample(audio, rate)
        assert got.shape == want.shape
        assert np.abs(got - want).max() < 1e-6


###############################################################################
# evaluation metrics against the reference's own run (tests/golden/metrics.npz)
###############################################################################


@pytest.mark.parametrize('loss', ['bce', 'mse'])
def test_metrics_restatement_matches_reference(loss):
    """oracle/metrics.py against what the reference's own `Statistics` /
    `Metrics.update` (evaluate/metrics.py:12-110) produced on seeded ragged
    batches: per-word BCE and squared-error values, per-batch and running
    results."""
    import os
    from oracle import metrics
    golden = np.load(os.path.join(
        os.path.dirname(__file__), 'golden', 'metrics.npz'))
    count = int(golden[f'{loss}/batches'])
    batches = [tuple(torch.from_numpy(golden[f'{loss}/{i}/{key}'])
                     for key in ('logits', 'targets', 'word_lengths'))
               for i in range(count)]
    predicted, target = [], []
    for logits, targets, lengths in batches:
        mask = metrics.mask_from_lengths(lengths)
        predicted += metrics.postprocess(logits, loss)[mask].tolist()
        target += targets[mask].tolist()
    stats_p, stats_t = metrics.mean_std(predicted), metrics.mean_std(target)
    np.testing.assert_allclose(stats_p, golden[f'{loss}/predicted_stats'], rtol=1e-12)
    np.testing.assert_allclose(stats_t, golden[f'{loss}/target_stats'], rtol=1e-12)
    total = metrics.Metrics(stats_p, stats_t, loss)
    for index, (logits, targets, lengths) in enumerate(batches):
        single = metrics.Metrics(stats_p, stats_t, loss)
        single.update(logits, targets, lengths)
        total.update(logits, targets, lengths)
        got = single()
        want = golden[f'{loss}/{index}/result']
        np.testing.assert_allclose(
            [got['pearson_correlation'], got['bce'], got['mse']], want,
            rtol=2e-6, atol=1e-7)
        values = metrics.word_values(logits, targets, lengths, loss)
        assert np.array_equal(values[0].numpy(), golden[f'{loss}/{index}/bce_values'])
        assert np.array_equal(
            values[1].numpy(), golden[f'{loss}/{index}/squared_errors'])
    got = total()
    np.testing.assert_allclose(
        [got['pearson_correlation'], got['bce'], got['mse']],
        golden[f'{loss}/result'], rtol=2e-6, atol=1e-7)


def test_whole_audio_features_match_reference(seams):
    """`data.preprocess.from_audio` / `mels.from_audio` / `loudness.from_audio`
    of the reference on WHOLE audios (tests/golden/generate.py seams; no
    zero-pad-and-slice in front) against the oracle's restatement."""
    switches = {
        'default': {}, 'normalized': {'normalize': True},
        'mel_loudness': {'loudness_feature': True},
        'loudness_normalized': {'mel_feature': False, 'loudness_feature': True,
                                'normalize': True}}
    for name in seams['audio/names']:
        audio = torch.from_numpy(seams[f'audio/{name}'])
        for tag, overrides in switches.items():
            want = seams[f'from_audio/{name}/{tag}']
            got = oracle.features(audio, overrides).numpy()
            assert got.shape == want.shape
            mels = 80 if overrides.get('mel_feature', True) else 0
            np.testing.assert_allclose(
                got[:, :mels], want[:, :mels], rtol=0, atol=1e-5)
            if overrides.get('loudness_feature'):
                tolerance = 2e-5 if overrides.get('normalize') else 1e-3
                np.testing.assert_allclose(
                    got[:, -1], want[:, -1], rtol=0, atol=tolerance)
        np.testing.assert_array_equal(
            seams[f'mels/{name}/default'], seams[f'from_audio/{name}/default'][0])
        np.testing.assert_array_equal(
            seams[f'loudness/{name}'],
            seams[f'from_audio/{name}/mel_loudness'][0, 80:])


###############################################################################
# the float64 oracle (the high-precision reference of tests/test_gpu_paths.py)
###############################################################################


@pytest.mark.parametrize('heads', [1, 2, 3, 4])
def test_float64_transformer_stack_matches_torch(heads):
    """`oracle.transformer_stack` in float64 against torch's own
    `nn.TransformerEncoderLayer` (post-LN, ReLU, eval) with the same weights:
    the independent check of the oracle's head split and key-padding mask."""
    from emphases_amd import config as cfg
    channels, length, layers = 120, 37, 2
    config = cfg.Config(architecture='transformer', channels=channels,
                        heads=heads, layers=layers)
    state = {k: torch.from_numpy(v).double()
             for k, v in weights.random_state(config, seed=11).items()}
    x = torch.from_numpy(synth.weights(5, (channels, length), 1.)).double()
    modules = []
    for i in range(layers):
        layer = torch.nn.TransformerEncoderLayer(
            channels, heads, dim_feedforward=channels, dropout=0.).double()
        prefix = f'frame_encoder.model.layers.{i}.'
        layer.load_state_dict({
            name: state[prefix + name] for name in layer.state_dict()})
        modules.append(layer.eval())
    for valid in (None, length, 23, 1):
        got = oracle.transformer_stack(
            x, state, 'frame_encoder', layers, heads, valid=valid)
        assert got.dtype == torch.float64
        h = (x.T + oracle.positional_encoding(
            length, channels, torch.float64))[:, None]        # [T, 1, C]
        mask = None
        if valid is not None:
            mask = torch.arange(length)[None] >= valid
        for layer in modules:
            h = layer(h, src_key_padding_mask=mask)
        assert torch.abs(got - h[:, 0].T).max() < 1e-12, (heads, valid)
    # the oracle's `stack` hands the configuration's heads through
    got = oracle.stack(x, state, 'frame_encoder', dict(
        architecture='transformer', layers=layers, heads=heads))
    want = oracle.transformer_stack(x, state, 'frame_encoder', layers, heads)
    assert torch.equal(got, want)


def test_float64_oracle_matches_variant_goldens(variants):
    """The oracle upcast to float64 (features, weights, word pieces,
    positional encoding) on every variant: within 1e-5 x scale of the
    float32 goldens - the upcast changed no arithmetic, only its precision."""
    audio = torch.from_numpy(synth.pcm_to_float(variants['audio_pcm']))
    bounds = variants['bounds_frames'].astype(np.int64)
    padded = torch.nn.functional.pad(audio, (432, 432))
    checked = 0
    for name in variants['names']:
        config, overrides = variant_config(name)
        state = {k: torch.from_numpy(v).double() for k, v in
                 variant_state(variants, name, config).items()}
        feats = oracle.features(
            padded[:, :audio.shape[1]], overrides, synth.pitch_tracks)[0]
        logits = oracle.forward(feats.double(), bounds, state, overrides)
        assert logits.dtype == torch.float64
        want = variants[f'{name}/logits']
        scale = float(np.abs(want).max())
        assert np.abs(logits.numpy() - want).max() < 1e-5 * scale, name
        checked += 1
    assert checked == 39


###############################################################################
# the float64 front-end (the reference of tests/test_gpu_frontend.py)
###############################################################################


def test_float64_frontend_matches_float32_on_seams(seams):
    """`logmel` / `loudness` / `features` follow the dtype of the audio; the
    float64 evaluation is the float32 one up to float32's own rounding."""
    for name in seams['audio/names']:
        audio = torch.from_numpy(seams[f'audio/{name}'])
        for normalize in (False, True):
            single = oracle.logmel(audio, normalize)
            double = oracle.logmel(audio.double(), normalize)
            assert single.dtype == torch.float32
            assert double.dtype == torch.float64
            assert float((single - double).abs().max()) < 1e-5
            single = oracle.loudness(audio, normalize)
            double = oracle.loudness(audio.double(), normalize)
            assert single.dtype == torch.float32
            assert double.dtype == torch.float64 and double.shape == single.shape
            assert float((single - double).abs().max()) < \
                (2e-7 if normalize else 2e-5)
        overrides = {'loudness_feature': True, 'pitch_feature': True}
        both = oracle.features(audio.double(), overrides, synth.pitch_tracks)
        assert both.dtype == torch.float64 and both.shape[1] == 82
        assert torch.equal(both[0, :80], oracle.logmel(audio.double()))
        assert torch.equal(both[0, 81:], oracle.loudness(audio.double()))
        single = oracle.features(audio, overrides, synth.pitch_tracks)
        assert single.dtype == torch.float32
        assert torch.equal(both[0, 80], single[0, 80].double())
        peak = oracle.peak_power(audio.double())
        assert peak == oracle.power(audio.double()).max()
        assert abs(float(oracle.peak_power(audio)) - peak) < 1e-6 * peak


def test_float64_frontend_uses_the_float32_constants():
    """Float64 arithmetic on the model's own float32 constants: the window
    torch builds in float32, the float32 mel basis, the A-weights as the engine
    uploads them."""
    from emphases_amd import engine, melbasis
    assert torch.equal(oracle.hann_window(torch.float64),
                       torch.hann_window(1024).double())
    assert np.array_equal(melbasis.default().dense, oracle.mel_basis().numpy())
    assert np.array_equal(
        engine.a_weighting(), oracle.a_weights(np.float32)[:, 0])
    # the device has ONE window table (halved: the 1/2 of the real-FFT split):
    # the loudness row's, the Hann evaluated in float64 and rounded once.  The
    # mel rows' window, evaluated by torch in float32, is up to 3 ulp from it
    # - which alone is up to 5e-6 on the metric of tests/frontend_signals.py
    # (the step), inside the device's budget there
    from emphases_amd import runtime
    table = 2. * np.asarray(runtime.frontend_table())[:1024]
    assert np.array_equal(table, oracle.loudness_window())
    gap = np.abs(table - oracle.hann_window().numpy())
    assert gap.max() <= 3 * 2. ** -24


def direct_dft(frame, bins):
    """sum_n frame[n] exp(-2 pi i k n / 1024) for k in bins: no FFT."""
    n = np.arange(1024)
    return np.array([
        np.sum(frame * np.exp(-2j * np.pi * ((k * n) % 1024) / 1024.))
        for k in bins])


def test_float64_frontend_closed_forms():
    """Answers that need no FFT, in float64, to 1e-12 (relative)."""
    basis = oracle.mel_basis().double()
    rowsum = basis.sum(dim=1)
    window = oracle.hann_window(torch.float64).numpy()
    weights_ = oracle.a_weights(np.float32).astype(np.float64)[:, 0]
    close = lambda got, want: np.testing.assert_allclose(   # noqa: E731
        np.asarray(got), np.asarray(want), rtol=1e-12, atol=0)

    # silence: every magnitude is sqrt(1e-6); every power clamps to 1e-10
    silence = torch.zeros(1, 4000, dtype=torch.float64)
    mel = oracle.logmel(silence)
    assert mel.shape == (80, 25)
    close(mel, torch.log(rowsum * 1e-3)[:, None].expand(80, 25))
    assert float(rowsum.min()) * 1e-3 > 6e-5          # the 1e-5 clamp is dead
    assert torch.equal(
        oracle.loudness(silence), torch.full((1, 25), -100., dtype=torch.float64))
    assert torch.equal(
        oracle.loudness(silence, True), torch.zeros(1, 25, dtype=torch.float64))
    assert oracle.peak_power(silence) == 0.

    # DC: X[k] = c sum_n w[n] exp(-2 pi i k n / 1024), the window's own sums
    for level in (32767. / 32768., -1., 1. / 32768.):
        dc = torch.full((1, 4000), level, dtype=torch.float64)
        want = np.abs(level * direct_dft(window, (0, 1)))
        close(want[0], abs(level) * window.sum())
        magnitude = oracle.magnitude(oracle.reflect_pad(dc))
        close(magnitude[:2, 7], np.sqrt(want ** 2 + 1e-6))
        # (the loudness row has a window of its own rounding)
        want = np.abs(level * direct_dft(
            oracle.loudness_window().astype(np.float64), (0, 1)))
        power = oracle.power(dc)
        close(power[:2, 7], want ** 2)
        close(oracle.peak_power(dc), want[0] ** 2)
        # bins 0 and 1 carry no mel weight but all of the loudness row: the rest
        # of the spectrum (the float32 window's rounding, 1e-14) sits on the
        # floor 80 dB under bin 0
        top = 10. * np.log10(max(1e-10, want[0] ** 2))
        db = np.full(513, top - 80.)
        db[:2] = np.maximum(10. * np.log10(np.maximum(1e-10, want ** 2)), top - 80.)
        close(oracle.loudness(dc)[0, 7], np.maximum(db + weights_, -100.).mean())

    # an impulse at the centre of frame 5's window: |X[k]| = w[512] = 1 flat
    impulse = torch.zeros(1, 4000, dtype=torch.float64)
    impulse[0, 80 + 160 * 5] = 1.
    assert window[512] == 1.
    magnitude = oracle.magnitude(oracle.reflect_pad(impulse))
    close(magnitude[:, 5], np.full(513, math.sqrt(1. + 1e-6)))
    close(oracle.mel(impulse)[:, 5], rowsum * math.sqrt(1. + 1e-6))
    np.testing.assert_allclose(oracle.power(impulse)[:, 5], 1., rtol=1e-12)
    # ... the chunk's peak, so the frame's row is the mean of the A-weights
    np.testing.assert_allclose(oracle.peak_power(impulse), 1., rtol=1e-12)
    np.testing.assert_allclose(
        oracle.loudness(impulse)[0, 5], weights_.mean(), rtol=0, atol=1e-11)
    # two frames on, the impulse sits at n = 192 of the window
    close(magnitude[:, 7], np.full(513, math.sqrt(window[192] ** 2 + 1e-6)))


###############################################################################
# does the front-end's budget tell a wrong kernel from a right one?
###############################################################################

MARGIN = 4.     # tests/test_gpu_frontend.py holds the device to MARGIN x floor


def mutated_mel(audio, basis=None, spectrum=None, repeat_edge=False):
    """`oracle.mel` in float64 with one fault planted."""
    if repeat_edge:
        x = audio[0]
        padded = torch.cat([x[:432].flip(0), x, x[-432:].flip(0)])
    else:
        padded = oracle.reflect_pad(audio)
    magnitude = oracle.magnitude(padded)
    if spectrum is not None:
        magnitude = spectrum(magnitude.clone())
    basis = oracle.mel_basis() if basis is None else basis
    return basis.double() @ magnitude


def basis_without(row, which):
    """The mel basis with one non-zero of `row` dropped: its first, or the
    middle one of its run."""
    basis = oracle.mel_basis().clone()
    bins = torch.nonzero(basis[row])[:, 0]
    basis[row, bins[0] if which == 'edge' else bins[len(bins) // 2]] = 0.
    return basis


def swap(target, source):
    def apply(magnitude):
        magnitude[target] = magnitude[source]
        return magnitude
    return apply


def halve(bin_):
    def apply(magnitude):
        magnitude[bin_] *= 0.5
        return magnitude
    return apply


def ripple(magnitude):
    """Every bin's magnitude off by a relative 2e-5: twiddle or window tables
    built in reduced precision look like this."""
    k = torch.arange(513, dtype=torch.float64)
    return magnitude * (1. + 2e-5 * torch.sin(1.7 * k))[:, None]


MEL_MUTATIONS = {
    'a weight dropped at a run\'s edge': dict(basis=('edge', 40)),
    'a weight dropped inside a run, row 70': dict(basis=('middle', 70)),
    'the basis shifted by one bin': dict(basis='shift'),
    'bin 256 halved': dict(spectrum=halve(256)),
    'bin 100 takes bin 101\'s value': dict(spectrum=swap(100, 101)),
    'reflect padding repeats the edge sample': dict(repeat_edge=True),
    'every bin off by a relative 2e-5': dict(spectrum=ripple)}


def test_mel_budget_discriminates():
    """Every planted fault is over MARGIN x floor on the metric of
    tests/frontend_signals.py on at least one signal - and the subtle one
    (2e-5 on every bin) moves `synth.audio(61)`'s log-mel by less than the 2e-5
    the log-domain tests allow."""
    import frontend_signals
    floors = frontend_signals.floors()
    floor = max(floors['mel', False], floors['mel', True])
    print(f'\nfloor: {floors["mel", False]:.2e} raw, '
          f'{floors["mel", True]:.2e} normalised; budget {MARGIN * floor:.2e}')
    # (what float32 arithmetic needs: 1e-6 raw; the normalised output's own
    # float32 rounding of (x + 10) / 10 is ten times that in the log)
    assert 5e-7 < floors['mel', False] < 5e-6 < floors['mel', True] < 3e-5
    signals = {name: frontend_signals.as_double(pcm)
               for name, pcm in frontend_signals.signals().items()}
    clean = {name: oracle.mel(audio) for name, audio in signals.items()}
    scale = {name: frontend_signals.mel_scale(audio)
             for name, audio in signals.items()}
    for title, mutation in MEL_MUTATIONS.items():
        mutation = dict(mutation)
        basis = mutation.pop('basis', None)
        if basis == 'shift':
            mutation['basis'] = torch.roll(oracle.mel_basis(), 1, dims=1)
        elif basis is not None:
            mutation['basis'] = basis_without(basis[1], basis[0])
        worst = {name: float(((mutated_mel(audio, **mutation) - clean[name])
                              .abs() / scale[name]).max())
                 for name, audio in signals.items()}
        name = max(worst, key=worst.get)
        print(f'{title}: {worst[name]:.2e} on {name} = '
              f'{worst[name] / (MARGIN * floor):.1f} x budget')
        assert worst[name] > MARGIN * floor, title
        if mutation.get('spectrum') is ripple:
            log = float((torch.log(mutated_mel(signals['synth61'], **mutation)) -
                         torch.log(clean['synth61'])).abs().max())
            print(f'    ... and {log:.2e} in synth61\'s log-mel')
            assert log < 2e-5
        elif basis is not None and basis != 'shift':
            # a misplaced weight shows where its bin leads the frame: the chirp
            assert worst['chirp'] > MARGIN * floor, title


def test_loudness_budget_discriminates():
    """The two faults the loudness row alone can show - bin 512 read from bin
    0, and a chunk's `top_db` floor hung on its neighbour's peak - against
    MARGIN x the float32 oracle's own gap, on the chunks of the multi-chunk
    batch of tests/test_gpu_frontend.py; and what chunk order that takes."""
    import frontend_signals
    floors = frontend_signals.floors()
    budget = MARGIN * max(floors['db', False], floors['db', True])
    print(f'\nfloor: {floors["db", False]:.2e} dB raw, '
          f'{floors["db", True]:.2e} dB normalised; budget {budget:.2e} dB')
    assert 1e-6 < budget < 1e-4
    chunks = frontend_signals.batch_chunks(cycles=1)
    powers = [oracle.power(frontend_signals.as_double(pcm))
              for _, pcm in chunks]
    peaks = [power.max() for power in powers]
    rows = [oracle.loudness_of_power(power) for power in powers]

    def moved(index, peak):
        return float((oracle.loudness_of_power(powers[index], peak=peak) -
                      rows[index]).abs().max())
    for index, (kind, _) in enumerate(chunks):
        for other in (index - 1, index + 1):
            if not 0 <= other < len(chunks):
                continue
            gap = moved(index, peaks[other])
            print(f'{kind} with the peak of {chunks[other][0]}: {gap:.1f} dB')
            assert gap > 1e4 * budget, (kind, chunks[other][0])
    # ... which is why no two quiet chunks are neighbours there: noise beside
    # silence hides a leak entirely
    quiet = [kind for kind, _ in chunks]
    noise, silence = quiet.index('lsb'), quiet.index('silence')
    assert moved(noise, peaks[silence]) == 0.
    assert moved(silence, peaks[noise]) == 0.
    # ... and why the short loud chunks are DC: three frames of a tone, all
    # reflections, have hardly a bin 80 dB under their peak for a lower floor
    # to free (0.0 to 0.1 dB with the tone's phase, against DC's 60)
    short = oracle.power(frontend_signals.as_double(
        frontend_signals.signals()['tone_between'][:481]))
    assert float((oracle.loudness_of_power(short, peak=peaks[noise]) -
                  oracle.loudness_of_power(short)).abs().max()) < 0.2
    # bin 512 taking bin 0's value: on the tones and the noise; silence has
    # nothing to show it with
    for (kind, _), power, row in zip(chunks, powers, rows):
        wrong = power.copy()
        wrong[512] = wrong[0]
        gap = float((oracle.loudness_of_power(wrong) - row).abs().max())
        print(f'{kind}, bin 512 <- bin 0: {gap:.2e} dB')
        assert (gap == 0.) if kind == 'silence' else gap > 10 * budget, kind
    blind = set()
    for name, pcm in frontend_signals.signals().items():
        power = oracle.power(frontend_signals.as_double(pcm))
        wrong = power.copy()
        wrong[512] = wrong[0]
        gap = float((oracle.loudness_of_power(wrong) -
                     oracle.loudness_of_power(power)).abs().max())
        print(f'{name}, bin 512 <- bin 0: {gap:.2e} dB')
        if gap <= 10 * budget:
            blind.add(name)
    # (flat spectra, and the tone on bin 256, as far from bin 0 as from bin
    # 512: both sit on the floor 80 dB under it)
    assert blind == {'silence', 'impulse', 'tone_bin256'}
