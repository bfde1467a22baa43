"""A float64 model of the PUSCH delay search (csrc/nr_delay.h) for the tests to hold the host form and the kernel to.

x: the reference's ul_ls_est of one antenna (nr_ul_channel_estimation.c:176-192 for type 1, :264-272 for type 2), restated here
with rx_chest_np.py's pilots and integer helpers -- as Python ints, so bit for bit -- indexed from the allocation's first RE, zero
from 12 nb_rb on, every antenna from zeros.  y = N ifft(x) = sum_k x[k] exp(+2 pi i k n / N) in float64, P = |y|^2.  The scan of
nr_est_delay (common/utils/nr/nr_common.c:968-990): n = 0 .. N - 1 with P > best from best = 0, position 0; position > N/2 has N
subtracted.  RUNNING_MAX (0) carries best and its position from antenna 0 on (the reference clears them once per call);
PER_ANTENNA (1) clears them per antenna.

Margin.  Next to every result the model returns 1 - sqrt(P_runner-up / P_winner) over all samples that compete for that entry: the
N samples of the antenna, and in RUNNING_MAX mode those of the antennas before it too.  A result whose margin exceeds the
transforms' errors is the same in fp32 and in float64.

B(N), the worst-case error of the fp32 transform relative to the peak's amplitude.  Higham, Accuracy and Stability of Numerical
Algorithms, 2nd ed., Thm 24.2: a radix-2 FFT of t = log2 N stages whose twiddles carry an error |w^ - w| <= mu gives
    ||y^ - y||_2 / ||y||_2 <= t eta / (1 - t eta),   eta = mu + gamma_4 (sqrt 2 + mu),  gamma_4 = 4u / (1 - 4u),
with u = 2^-24.  The proof bounds each stage (a butterfly = one complex multiplication by a twiddle and one complex addition, the
stage matrix of norm sqrt 2) by eta relative to that norm and is the same for the decimation-in-frequency factorisation used here,
which is the transposed product.  The twiddles are computed in double and rounded once, so each component is off by at most u of
its size and |w^ - w| <= u (1 + 2^-28); mu = 2u leaves room.  The radix-3 stage of 1536 and 6144 forms ((a + b w') + c w'') w:
two levels of multiply-and-add and one more multiplication, each within eta, so it counts as three stages: t = log2 N for a power
of two, log2(N / 3) + 3 otherwise.  A single sample is off by at most the whole vector's error,
    |y^[n] - y[n]| <= t eta ||y||_2 / (1 - t eta) = t eta sqrt N ||x||_2 / (1 - t eta),
and the peak is at least the root mean square, |y[peak]| >= ||y||_2 / sqrt N = ||x||_2.  So every sample's error is at most
    B(N) = t eta sqrt N / (1 - t eta)
of the peak's amplitude: 3.6e-5 at 128, 5.4e-4 at 8192.  Two samples whose amplitudes differ by more than 2 B(N) of the larger keep
their order in fp32; the |.|^2 (two roundings of products, one of the sum: 2u of the amplitude) and the reduction (comparisons:
exact) add nothing comparable.  The tests require a margin of 8 B(N) of every case, and hold peaks to the model within B(N) of the
amplitude.
"""
import math

import numpy as np

import rx_chest_np as R

RUNNING_MAX, PER_ANTENNA = 0, 1
# misreadings of the definition that the cases of test_rx_delay_host.py must notice
MISREADINGS = ("exponent_sign", "fold_ge", "mode_swapped", "grid_indexed", "own_res", "t2_drop45", "delta_ignored", "antennas_swapped")


def stages(N):
    return int(math.log2(N // 3)) + 3 if N % 3 == 0 else int(math.log2(N))


def B(N):
    u = 2.0 ** -24
    mu = 2 * u
    eta = mu + 4 * u / (1 - 4 * u) * (math.sqrt(2.0) + mu)
    t = stages(N)
    return t * eta * math.sqrt(N) / (1 - t * eta)


def ls_est(rx, soffset, N, k0, nb_rb, p, dmrs_type, c_init, re_offset, mis=frozenset()):
    """ul_ls_est of one antenna: N pairs of ints.  rx = the antenna's buffer as pairs, soffset = the symbol's subcarrier 0"""
    pilot = R.pusch_dmrs_rx(c_init, p, nb_rb, re_offset, dmrs_type)
    shift = 0 if "delta_ignored" in mis else (p >> 1) & 1      # delta (type 1: in the RE index) = nushift (type 2: behind the wrap)
    x = [(0, 0)] * N
    if dmrs_type == 0:
        for n in range(3 * nb_rb):                                                           # :176
            ch = (0, 0)
            for k_line in range(2):
                re = (k0 + (n << 2) + (k_line << 1) + shift) % N                             # :181
                t = R.c32_mul_shift(pilot[2 * n + k_line], rx[soffset + re], 16)
                if "own_res" in mis:
                    x[4 * n + 2 * k_line + shift] = (R.s16(t[0] * 2), R.s16(t[1] * 2))
                ch = (ch[0] + t[0], ch[1] + t[1])
            if "own_res" not in mis:
                for j in range(4):                                                           # :188-190
                    x[4 * n + j] = (R.s16(ch[0]), R.s16(ch[1]))
    else:
        for m in range(2 * nb_rb):                                                           # :263
            ch0 = R.c16_mul_shift(pilot[2 * m], rx[soffset + shift + (k0 + 6 * m) % N], 15)
            ch1 = R.c16_mul_shift(pilot[2 * m + 1], rx[soffset + shift + (k0 + 6 * m + 1) % N], 15)
            ch = (R.s16((ch0[0] + ch1[0]) >> 1), R.s16((ch0[1] + ch1[1]) >> 1))
            if "own_res" in mis:
                x[6 * m], x[6 * m + 1] = ch0, ch1
                continue
            low = tuple(R.sat16(R.sat16(0 + R.s16(((c * 16384) >> 16) << 2)) + 0) for c in ch)   # :270 on zeros: mulhi_s1, two adds
            for j in range(4):
                x[6 * m + j] = low
            if "t2_drop45" not in mis:
                x[6 * m + 4] = x[6 * m + 5] = ch                                             # :271-272
    if "grid_indexed" in mis:
        x = [x[(k - k0) % N] for k in range(N)]
    return x


def power(x, N, mis=frozenset()):
    z = np.array([complex(r, i) for r, i in x], np.complex128)
    y = np.fft.fft(z) if "exponent_sign" in mis else np.fft.ifft(z) * N
    return y.real ** 2 + y.imag ** 2


def fold(pos, N, mis=frozenset()):
    return pos - N if (pos >= N // 2 if "fold_ge" in mis else pos > N // 2) else pos


def scan(P_ants, N, flags, mis=frozenset()):
    """P_ants = one power array per antenna -> (delays, peaks, margins) per antenna"""
    if "mode_swapped" in mis:
        flags = 1 - flags
    if "antennas_swapped" in mis:
        P_ants = P_ants[::-1]
    delays, peaks, margins = [], [], []
    best, pos, seen = 0.0, 0, []
    for P in P_ants:
        if flags == PER_ANTENNA:
            best, pos, seen = 0.0, 0, []
        for n in range(N):                                                                   # nr_common.c:975-981
            if P[n] > best:
                best, pos = float(P[n]), n
        seen.append(np.asarray(P))
        allp = np.sort(np.concatenate(seen))
        margins.append(1.0 - math.sqrt(allp[-2] / allp[-1]) if allp[-1] > 0 else 1.0)
        delays.append(fold(pos, N, mis))
        peaks.append(best)
    if "antennas_swapped" in mis:
        delays, peaks, margins = delays[::-1], peaks[::-1], margins[::-1]
    return delays, peaks, margins


def est_delay(rx_ants, seg, flags, mis=frozenset()):
    """one descriptor (a dict with the fields of nrLDPC_hip_chest_seg_t; rx_off = the symbol's offset in each antenna's buffer of
    pairs) -> (delays, peaks, margins) per antenna; the averaging modes take no delay"""
    n_rx, N = len(rx_ants), seg["fft_size"]
    if seg["mode"] >> 1:
        return [0] * n_rx, [0.0] * n_rx, [1.0] * n_rx
    re_offset = seg["dmrs_offset"] * (3 if seg["mode"] & 1 else 2)                           # nr_dmrs_rx.c:84 back
    P = [power(ls_est(rx, seg["rx_off"], N, seg["start_re"], seg["rb_size"], seg["port"], seg["mode"] & 1, seg["c_init"], re_offset, mis), N, mis)
         for rx in rx_ants]
    return scan(P, N, flags, mis)
