"""Helpers of the preprocessing tests: the numpy restatement of
`emph_unpack_rows`, WAVE writers for the sample formats the tests need, and
a minimal TextGrid."""
import struct

import numpy as np


def gather(x, table, out):
    """`emph_unpack_rows` in numpy: entry (column, frames, row, rows, target)
    writes out[target + r * frames + f] = x[row + r, column + f]; `x` is the
    packed matrix [rows, ld], `out` the flat destination (changed in place)."""
    for column, frames, row, rows, target in np.asarray(table).tolist():
        block = x[row:row + rows, column:column + frames]
        out[target:target + rows * frames] = block.reshape(-1)
    return out


def blocks(table, flat):
    """The [rows, frames] tensors a table's entries name in `flat`."""
    return [flat[target:target + rows * frames].reshape(rows, frames)
            for _, frames, _, rows, target in np.asarray(table).tolist()]


def _riff(fmt, body):
    chunks = b'fmt ' + struct.pack('<I', len(fmt)) + fmt + \
        b'data' + struct.pack('<I', len(body)) + body
    return b'RIFF' + struct.pack('<I', 4 + len(chunks)) + b'WAVE' + chunks


def write_float_wav(path, audio, rate=16000):
    """float32 [channels, samples] as an IEEE-float WAVE file, bit for bit."""
    audio = np.asarray(audio, dtype='<f4')
    audio = audio[None] if audio.ndim == 1 else audio
    channels = audio.shape[0]
    fmt = struct.pack('<HHIIHH', 3, channels, rate, rate * channels * 4,
                      channels * 4, 32)
    with open(path, 'wb') as file:
        file.write(_riff(fmt, np.ascontiguousarray(audio.T).tobytes()))


def write_pcm_wav(path, pcm, rate=16000):
    """int16 [channels, samples] as a 16-bit PCM WAVE file, bit for bit."""
    pcm = np.asarray(pcm, dtype='<i2')
    pcm = pcm[None] if pcm.ndim == 1 else pcm
    channels = pcm.shape[0]
    fmt = struct.pack('<HHIIHH', 1, channels, rate, rate * channels * 2,
                      channels * 2, 16)
    with open(path, 'wb') as file:
        file.write(_riff(fmt, np.ascontiguousarray(pcm.T).tobytes()))


def to_pcm(audio):
    """float audio -> int16 (round, clip)."""
    return np.clip(np.rint(np.asarray(audio, dtype=np.float64) * 32768.),
                   -32768, 32767).astype(np.int16)


TEXTGRID = '''File type = "ooTextFile"
Object class = "TextGrid"

xmin = 0
xmax = 1
tiers? <exists>
size = 1
item []:
    item [1]:
        class = "IntervalTier"
        name = "words"
        xmin = 0
        xmax = 1
        intervals: size = 1
        intervals [1]:
            xmin = 0
            xmax = 1
            text = "a"
'''
