"""Shared by tests/test_cpu_codec*.py and tests/test_gpu_codec*.py: a word-level model of the device range encoder
(csrc/pc_encode.hip) in plain Python, the host coder wrapped so that its pending-underflow count can be observed, and the
constructed sequences (long pending runs, worst-case cost) as logits whose softmax tables give them.  For the decoders: a
word-level model of pc_dec_symbol_wave (csrc/pc_decode.hip), the host decoder as a function of (bytes, tables), context-model
weights whose table is one chosen row at every position, and the byte strings no encoder wrote."""
import io

import numpy as np

from imgcomp_cvpr_amd import arithmetic_coding as ac

M32 = 0xffffffff


def clz32(x):
    return 32 - int(x).bit_length()


class ModelSink(object):
    """PceSink: a 64-bit reservoir flushed in whole bytes; a run longer than the reservoir leaves as whole bytes."""

    def __init__(self, capacity=None):
        self.buf = bytearray()
        self.res, self.nres, self.ovf, self.cap = 0, 0, False, capacity

    def put(self, bits, k):
        assert 0 <= k <= 56 and 0 <= bits < (1 << k) and self.nres < 8
        if self.ovf:
            return
        self.res = (self.res << k) | bits
        assert self.res < (1 << 64)                              # the kernel's reservoir is 64 bits wide
        self.nres += k
        if self.nres >= 8:
            nb, rem = self.nres >> 3, self.nres & 7
            if self.cap is not None and len(self.buf) + nb > self.cap:
                self.ovf = True
                return
            for lane in range(nb):
                self.buf.append((self.res >> (rem + 8 * (nb - 1 - lane))) & 0xff)
            self.nres = rem
            self.res &= (1 << rem) - 1

    def put_run(self, bit, p):
        ones = (1 << 64) - 1 if bit else 0
        if p <= 48:
            self.put(ones & ((1 << p) - 1), p)
            return
        k = 8 - self.nres
        self.put(ones & ((1 << k) - 1), k)
        p -= k
        if self.ovf:
            return
        nb = p >> 3
        if self.cap is not None and len(self.buf) + nb > self.cap:
            self.ovf = True
            return
        self.buf.extend(bytes([ones & 0xff]) * nb)
        t = p & 7
        self.put(ones & ((1 << t) - 1), t)


def model_div(n, d):
    """pce_div: the double-precision product with the reciprocal, then one exact correction step."""
    q = int(float(n) * (1.0 / float(d)))
    rem = n - q * d
    if rem < 0:
        q -= 1
    elif rem >= d:
        q += 1
    return q


def model_encode(cum_lo, cum_hi, total, capacity=None):
    """the kernel's serial loop over (cum_lo, cum_hi, total) triples -> (bytes, status, largest pending run)."""
    o = ModelSink(capacity)
    low, high, pending, max_pending = 0, M32, 0, 0
    for lo, hi, tot in zip(cum_lo, cum_hi, total):
        lo, hi, tot = int(lo), int(hi), int(tot)
        if tot > ac.MAX_TOTAL:
            return bytes(o.buf), 1, max_pending
        r = high - low + 1
        qh, ql = model_div(hi * r, tot), model_div(lo * r, tot)
        assert qh == hi * r // tot and ql == lo * r // tot
        high = (low + qh - 1) & M32
        low = (low + ql) & M32
        x = low ^ high
        n = clz32(x) if x else 32
        if n:
            top = low >> (32 - n)
            if pending == 0:
                o.put(top, n)
            else:
                bit = low >> 31
                o.put(bit, 1)
                o.put_run(bit ^ 1, pending)
                pending = 0
                o.put(top & ((1 << (n - 1)) - 1), n - 1)
            low = (low << n) & M32
            high = ((high << n) | ((1 << n) - 1)) & M32
            if o.ovf:
                break
        y = ((low & ~high) << 1) & M32
        m = clz32(~y & M32)
        if m:
            pending += m
            max_pending = max(max_pending, pending)
            low = (low << m) & 0x7fffffff
            high = ((high << m) & 0x7fffffff) | 0x80000000 | ((1 << m) - 1)
    o.put(1, 1)
    if o.nres:
        o.put(0, 8 - o.nres)
    return bytes(o.buf), (2 if o.ovf else 0), max_pending


def triples(symbols, freqs):
    symbols = np.asarray(symbols).astype(np.int64)
    cum = np.concatenate([np.zeros((len(freqs), 1), np.int64), np.cumsum(np.asarray(freqs).astype(np.int64), axis=1)], axis=1)
    idx = np.arange(len(symbols))
    return cum[idx, symbols].tolist(), cum[idx, symbols + 1].tolist(), cum[:, -1].tolist()


class _Keep(io.BytesIO):
    def close(self):
        self.kept = self.getvalue()
        io.BytesIO.close(self)


def host_encode(symbols, freqs):
    """arithmetic_coding's coder, symbol by symbol -> (bytes, the largest value its _pending reached)."""
    buf = _Keep()
    out = ac.CountingBitOutputStream(ac.BitOutputStream(buf))
    enc = ac.ArithmeticEncoder(out)
    max_pending = 0
    for lo, hi, tot in zip(*triples(symbols, freqs)):
        enc.write_cum(lo, hi, tot)
        max_pending = max(max_pending, enc._pending)
    enc.finish()
    out.close()
    assert out.num_bits == 8 * len(buf.kept)
    return buf.kept, max_pending


def softmax_tables(logits, resolution=1e9):
    """max(int64(softmax * resolution), 1) in fp32, the expression of pc_table_row (numpy's expf may differ from the device's in
    the last place: a GPU test takes its tables from the device, this one serves the CPU tests and the construction below)."""
    l = np.asarray(logits, np.float32)
    e = np.exp(l - l.max(axis=1, keepdims=True), dtype=np.float32)
    s = np.zeros(len(l), np.float32)
    for j in range(l.shape[1]):
        s = s + e[:, j]
    p = (e / s[:, None]).astype(np.float32)
    return np.maximum((p * np.float32(resolution)).astype(np.int64), 1)


PENDING_SEED = 20240607
PENDING_L = 16


def pending_run_logits(steps=80, tail=40, seed=PENDING_SEED):
    """-> (logits (n, 16) float32, symbols (n,)), found by a greedy search that follows the host coder's state: every step picks,
    among the tables "j symbols of logit 0, the others of logit -1000" (j = 2..16) and their symbols, the one whose interval
    straddles 2^31 most evenly -- low = 01.., high = 10..: underflow bits and never a shift, so the pending run grows with every
    symbol.  These tables are the same on every implementation (exp(0) = 1 and exp(-1000) = 0 exactly, j ones summed exactly, one
    IEEE division: fp32(1 / j) * 1e9 truncated, the other symbols at the floor of 1), so the search done on the host holds for
    the tables the device derives.  `tail` seeded random symbols then release the run."""
    rs = np.random.RandomState(seed)
    enc = ac.ArithmeticEncoder(ac.CountingBitOutputStream(ac.BitOutputStream(_Keep())))
    rows = {j: np.array([0.0] * j + [-1000.0] * (PENDING_L - j), np.float32) for j in range(2, PENDING_L + 1)}
    cums = {j: np.concatenate([[0], np.cumsum(softmax_tables(rows[j][None])[0])]) for j in rows}
    logits, symbols = [], []
    half = 1 << 31
    for _ in range(steps):
        r = enc.high - enc.low + 1
        best = None
        for j, cum in cums.items():
            tot = int(cum[-1])
            for k in range(j):
                lo, hi = enc.low + int(cum[k]) * r // tot, enc.low + int(cum[k + 1]) * r // tot - 1
                score = min(half - lo, hi - half + 1) / float(hi - lo + 1)          # 0.5 = centred on 2^31, <= 0 = no straddle
                if best is None or score > best[0]:
                    best = (score, j, k)
        score, j, k = best
        assert score > 0, 'no table straddles 2^31'
        enc.write_cum(int(cums[j][k]), int(cums[j][k + 1]), int(cums[j][-1]))
        logits.append(rows[j])
        symbols.append(k)
    for _ in range(tail):
        logits.append(rs.uniform(0, 3, size=PENDING_L).astype(np.float32))
        symbols.append(int(rs.randint(PENDING_L)))
    return np.stack(logits), np.array(symbols, np.int64)


def worst_case_logits(n=200):
    """the symbol of frequency 1 (p = e^-40 truncates to 0, floor 1) against one of frequency `resolution`, repeated:
    about log2(1e9 + 1) = 29.9 bits per symbol, the most a softmax table can cost."""
    return np.tile(np.array([[0.0, 40.0]], np.float32), (n, 1)), np.zeros(n, np.int64)


# ---- the decode side ----------------------------------------------------------------------------------------------------------

LAST_LAYER = 'probclass3d/logits/conv3d_conv2_mask'


def constant_table_weights(ae_cfg, pc_cfg, bias, seed=1234):
    """weights.synthetic_weights with the filter of the last context-model layer zeroed and its bias set to `bias`.  The logits of
    a position are relu(conv(activations, filter) + bias); every product with a zero filter tap is +-0 (the activations are
    finite), their sum is +-0, +-0 + bias is bias exactly and bias >= 0 passes the ReLU unchanged: the logits are exactly `bias`
    at every position, whatever the symbols around it and whichever kernel computes them (parallel pass, encoder, every decoder).
    The frequency table is then one row, chosen by the test."""
    from imgcomp_cvpr_amd import weights as W
    bias = np.asarray(bias, np.float32)
    assert bias.shape == (ae_cfg.num_centers,) and (bias >= 0).all(), 'one bias per centre, none below 0 (the final ReLU)'
    w = W.synthetic_weights(ae_cfg, pc_cfg, seed=seed)
    w[LAST_LAYER + '/weights'] = np.zeros_like(w[LAST_LAYER + '/weights'])
    w[LAST_LAYER + '/biases'] = bias.copy()
    return w


def straddle_symbols(table, steps, prefix=()):
    """one fixed integer table: after coding `prefix`, follow the host encoder's state and always code the symbol whose interval
    contains 2^31 (lo < 2^31 <= hi) -- its top bits differ, nothing is shifted out, so the pending count only grows.
    -> (the `steps` symbols, the pending count reached).  A table without such a symbol at some step (a cumulative boundary
    exactly at half the range) is refused."""
    table = [int(v) for v in table]
    cum = [0]
    for v in table:
        cum.append(cum[-1] + v)
    tot = cum[-1]
    enc = ac.ArithmeticEncoder(ac.CountingBitOutputStream(ac.BitOutputStream(_Keep())))
    for k in prefix:
        enc.write_cum(cum[k], cum[k + 1], tot)
    half, symbols = 1 << 31, []
    for step in range(steps):
        r = enc.high - enc.low + 1
        hit = [k for k in range(len(table))
               if enc.low + cum[k] * r // tot < half <= enc.low + cum[k + 1] * r // tot - 1]
        assert len(hit) == 1, 'table {}: no symbol straddles 2^31 at step {} (low {:#x}, high {:#x})'.format(table, step, enc.low, enc.high)
        before = enc._pending
        enc.write_cum(cum[hit[0]], cum[hit[0] + 1], tot)
        assert enc._pending >= before
        symbols.append(hit[0])
    return symbols, enc._pending


def _freq_tables(freq_rows):
    """one SimpleFrequencyTable per row; a row that is the same object as the one before it (a constant table repeated) shares it"""
    last, table = None, None
    for row in freq_rows:
        if table is None or row is not last:
            last, table = row, ac.SimpleFrequencyTable(row)
        yield table


def host_decode(data, freq_rows):
    """arithmetic_coding's decoder over the bytes `data`, one table per symbol -> list of symbols.  It reads zeros past the end
    and never refuses a byte string: a total reference for streams that no encoder wrote."""
    dec = ac.ArithmeticDecoder(ac.BitInputStream(io.BytesIO(bytes(data))))
    return [dec.read(t) for t in _freq_tables(freq_rows)]


def model_udiv(n, d):
    """pc_udiv: the double-precision quotient, then one exact correction step.  Its documented precondition: n < 2^63,
    d < 2^34, n / d < 2^34."""
    assert 0 <= n < (1 << 63) and 0 < d < (1 << 34) and n // d < (1 << 34)
    q = int(float(n) / float(d))
    rem = n - q * d
    if rem < 0:
        q -= 1
    elif rem >= d:
        q += 1
    return q


class ModelBits(object):
    """pc_dec_bit: most significant bit first, zeros past the end"""

    def __init__(self, data):
        self.data, self.pos, self.left, self.cur = bytes(data), -1, 0, 0

    def bit(self):
        if self.left == 0:
            self.pos += 1
            self.cur = self.data[self.pos] if self.pos < len(self.data) else 0
            self.left = 8
        self.left -= 1
        return (self.cur >> self.left) & 1


def model_decode(data, freq_rows):
    """pc_dec_symbol_wave's serial loop over the tables -> (symbols, status): the 32 priming bits, value by pc_udiv, the linear
    search over the cumulative sums, both renormalisation loops.  status 1 (and the symbols before) at the first table whose
    total exceeds 2^30 + 2."""
    TOP, SECOND = 1 << 31, 1 << 30
    inp = ModelBits(data)
    low, high, code = 0, M32, 0
    for _ in range(32):
        code = (code << 1) | inp.bit()
    symbols = []
    for row in freq_rows:
        fr = [int(v) for v in row]
        L, total = len(fr), sum(fr)
        if total > ac.MAX_TOTAL:
            return symbols, 1
        assert low <= code <= high
        r = high - low + 1
        value = model_udiv((code - low + 1) * total - 1, r)
        assert value == ((code - low + 1) * total - 1) // r
        sym, cum = 0, 0
        while sym + 1 < L and cum + fr[sym] <= value:
            cum += fr[sym]
            sym += 1
        qh, ql = model_udiv((cum + fr[sym]) * r, total), model_udiv(cum * r, total)
        assert qh == (cum + fr[sym]) * r // total and ql == cum * r // total
        high = low + qh - 1
        low = low + ql
        while ((low ^ high) & TOP) == 0:
            code = ((code << 1) & M32) | inp.bit()
            low = (low << 1) & M32
            high = ((high << 1) & M32) | 1
        while (low & ~high & SECOND) != 0:
            code = (code & TOP) | ((code << 1) & (M32 >> 1)) | inp.bit()
            low = (low << 1) & (M32 >> 1)
            high = ((high << 1) & (M32 >> 1)) | TOP | 1
        symbols.append(sym)
    return symbols, 0


def garbage_strings(valid, seed, lengths=(1, 7, 64, 200)):
    """byte strings that no encoder wrote, for a decoder that must still agree with the host decoder on them:
    [(name, bytes)] -- empty, all ones, all zeros, zeros then ones, seeded random strings of `lengths`, and the valid stream
    `valid` cut at each of its first 16 byte positions, cut in half, and with one bit flipped (early, in the middle, at the end)."""
    rs = np.random.RandomState(seed)
    out = [('empty', b''), ('ones', b'\xff' * 64), ('zeros', b'\x00' * 64), ('zeros then ones', b'\x00' * 4 + b'\xff' * 60)]
    out += [('random {}'.format(n), rs.randint(0, 256, size=n).astype(np.uint8).tobytes()) for n in lengths]
    out += [('cut at {}'.format(n), valid[:n]) for n in range(min(16, len(valid)))]
    out.append(('first half', valid[:len(valid) // 2]))
    for bit in sorted(set([3, 4 * len(valid), 8 * len(valid) - 1, int(rs.randint(0, 8 * len(valid)))])) if valid else []:
        flipped = bytearray(valid)
        flipped[bit >> 3] ^= 0x80 >> (bit & 7)
        out.append(('bit {} flipped'.format(bit), bytes(flipped)))
    return out
