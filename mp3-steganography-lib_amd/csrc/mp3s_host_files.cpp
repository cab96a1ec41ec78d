// Container formats and message framing on the host: WAV header in/out, "<count>#<text>" framing
// and the reveal parse.  Byte shuffling only -- nothing here is on the device path.
#include <stdio.h>
#include <math.h>
#include <string.h>
#include <map>
#include <mutex>

#include "mp3s_host.h"

namespace mp3s {
namespace {

long find4(const uint8_t *buf, size_t n, const char *tag)
{
    for (size_t i = 0; i + 4 <= n; i++)
        if (!memcmp(buf + i, tag, 4)) return (long)i;
    return -1;
}

// struct.unpack on a slice of the 128-byte header buffer: a short slice is a struct.error in the reference
bool le(const uint8_t *buf, size_t n, long at, int bytes, uint32_t *v)
{
    if (at < 0 || (size_t)at + bytes > n) return false;
    uint32_t x = 0;
    for (int i = 0; i < bytes; i++) x |= (uint32_t)buf[at + i] << (8 * i);
    *v = x;
    return true;
}

bool is_space(uint8_t c)   // what int() strips below code point 256: C isspace plus NEL and NBSP (not 0x1c..0x1f)
{
    return (c >= 0x09 && c <= 0x0d) || c == 0x20 || c == 0x85 || c == 0xa0;
}

// int(text) of CPython for a string of code points < 256: surrounding whitespace, one sign, decimal digits with single
// underscores between them.  Saturates at +-2^62 (a length that large only decides "longer than the text").
bool py_int(const uint8_t *s, size_t n, int64_t *out)
{
    size_t a = 0, b = n;
    while (a < b && is_space(s[a])) a++;
    while (b > a && is_space(s[b - 1])) b--;
    bool neg = false;
    if (a < b && (s[a] == '+' || s[a] == '-')) neg = s[a++] == '-';
    if (a == b) return false;
    int64_t v = 0;
    bool prev_digit = false;
    for (size_t i = a; i < b; i++) {
        if (s[i] == '_') {
            if (!prev_digit || i + 1 == b) return false;
            prev_digit = false;
            continue;
        }
        if (s[i] < '0' || s[i] > '9') return false;
        if (v < ((int64_t)1 << 58)) v = v * 10 + (s[i] - '0');
        else v = (int64_t)1 << 62;
        prev_digit = true;
    }
    *out = neg ? -v : v;
    return true;
}

}  // namespace

// reference encoder/WAV_Reader.py:30-107 (+ check_bitrate_index :109-111).  Returns MP3S_OK, MP3S_E_EXIT with the
// reference's sys.exit text in *msg, or MP3S_E_MALFORMED where the reference dies in struct.unpack / a division.
int wav_parse(const uint8_t *file, size_t len, int bitrate_kbps, mp3s_wav_info *o, const char **msg)
{
    const size_t n = len < 128 ? len : 128;   // the header is searched in the first 128 bytes only
    uint32_t v = 0;
    *msg = "Bad WAVE file.";
    long idx = find4(file, n, "RIFF");
    if (idx < 0) return MP3S_E_EXIT;
    *msg = "short WAVE header";
    if (!le(file, n, idx + 4, 4, &v)) return MP3S_E_MALFORMED;
    *msg = "Bad WAVE file.";
    if (find4(file, n, "WAVE") < 0) return MP3S_E_EXIT;
    idx = find4(file, n, "fmt ");
    if (idx < 0) return MP3S_E_EXIT;
    idx += 4;
    *msg = "short WAVE header";
    if (!le(file, n, idx, 4, &v)) return MP3S_E_MALFORMED;
    *msg = "Unsupported WAVE file, compression used instead of PCM.";
    if (v != 16) return MP3S_E_EXIT;
    idx += 4;
    if (!le(file, n, idx, 2, &v)) { *msg = "short WAVE header"; return MP3S_E_MALFORMED; }
    if (v != 1) return MP3S_E_EXIT;
    idx += 2;
    *msg = "short WAVE header";
    if (!le(file, n, idx, 2, &v)) return MP3S_E_MALFORMED;
    o->channels = (int32_t)v;
    idx += 2;
    if (!le(file, n, idx, 4, &v)) return MP3S_E_MALFORMED;
    o->samplerate = (int32_t)v;
    *msg = "Unsupported sampling frequency.";
    if (v != 32000 && v != 44100 && v != 48000) return MP3S_E_EXIT;
    idx += 4 + 4 + 2;   // byte rate and block align are read but never used
    *msg = "short WAVE header";
    if (!le(file, n, idx, 2, &v)) return MP3S_E_MALFORMED;
    o->bits_per_sample = (int32_t)v;
    *msg = "Unsupported WAVE file, samples not int8, int16 or int32 type.";
    if (v != 8 && v != 16 && v != 32) return MP3S_E_EXIT;
    *msg = "Bad WAVE file.";
    idx = find4(file, n, "data");
    if (idx < 0) return MP3S_E_EXIT;
    idx += 4;
    *msg = "short WAVE header";
    if (!le(file, n, idx, 4, &v)) return MP3S_E_MALFORMED;
    *msg = "WAVE header with zero channels (ZeroDivisionError in the reference)";
    if (o->channels == 0) return MP3S_E_MALFORMED;
    // int(sub_chunk2_size * 8 / bits_per_sample / channels): two float divisions, truncation
    o->num_of_samples = (int64_t)((double)((uint64_t)v * 8) / (double)o->bits_per_sample / (double)o->channels);
    o->data_offset = idx + 4;
    // np.fromfile(f, 'int16', num_of_samples * channels * 2): always int16, up to TWICE the declared values, cut by EOF
    const int64_t want = o->num_of_samples * o->channels * 2;
    const int64_t have = (size_t)o->data_offset <= len ? (int64_t)((len - (size_t)o->data_offset) / 2) : 0;
    o->n_values = want < have ? want : have;
    o->bitrate = bitrate_kbps;
    int sri, bri, whole;
    *msg = "Unsupported bitrate configuration.";
    if (stream_params(o->samplerate, bitrate_kbps, &sri, &bri, &whole)) return MP3S_E_EXIT;
    *msg = "";
    return MP3S_OK;
}

int wav_frame_count(const mp3s_wav_info &w, int64_t *count_out, const char **msg)
{
    // MP3_Encoder.py:596-618 walks num_of_samples * channels values in steps of 1152 * channels and indexes the buffer
    // as if it were stereo: mono input and a partial last frame both end in IndexError there
    *count_out = 0;
    *msg = "mono input: the reference encoder indexes the sample buffer out of bounds";
    if (w.channels != 2) return MP3S_E_UNSUPPORTED;
    // count whole frames, plus one more when samples are left over (:611-614): that frame is read from whatever follows in
    // the buffer -- np.fromfile was asked for twice the declared count (WAV_Reader.py:108), so a chunk behind the data
    // chunk, or the second half of samples that are not 16 bits wide, is taken for audio; only a buffer that ends inside
    // the frame raises (IndexError)
    const int64_t total = w.num_of_samples * 2;
    const int64_t count = total / 2304 + (total % 2304 ? 1 : 0);
    *msg = "sample count is not a multiple of 1152 per channel and the file ends inside the last frame: the reference encoder reads past the end of the sample buffer";
    if (count <= 0 || w.n_values < count * 2304) return MP3S_E_UNSUPPORTED;
    *count_out = count;
    *msg = "";
    return MP3S_OK;
}

// The opt-in reader (MP3S_OPT_WAV_IMPORT; the rules are stated at mp3s_wav_import_info in include/mp3s.h): a RIFF chunk walk over the
// whole file instead of a tag search in its first 128 bytes, and every sample format a WAV file usually has.  The reference's texts
// are kept for what both readers refuse.
int wav_import_parse(const uint8_t *file, size_t len, int bitrate_kbps, mp3s_wav_import *o, const char **msg, int resample, mp3s_wav_resample *rs)
{
    memset(o, 0, sizeof *o);
    if (rs) memset(rs, 0, sizeof *rs);
    int out_rate = 0, rL = 1, rM = 1, rT = 0, rH = 0;
    *msg = "Bad WAVE file.";
    if (len < 12 || memcmp(file, "RIFF", 4) || memcmp(file + 8, "WAVE", 4)) return MP3S_E_EXIT;
    uint64_t fmt_at = 0, fmt_size = 0, data_at = 0, data_size = 0;
    bool have_fmt = false, have_data = false;
    for (uint64_t pos = 12; pos + 8 <= len;) {   // (a chunk header cut by the end of the file ends the walk)
        uint32_t size = 0;
        le(file, len, (long)pos + 4, 4, &size);
        if (!memcmp(file + pos, "data", 4)) {
            if (!have_fmt) return MP3S_E_EXIT;
            have_data = true; data_at = pos + 8; data_size = size;
            break;
        }
        if (!have_fmt && !memcmp(file + pos, "fmt ", 4)) { have_fmt = true; fmt_at = pos + 8; fmt_size = size; }
        pos += 8 + (uint64_t)size;
        // the pad byte of an odd chunk is zero; a writer that left it out (the reference's reader never asked for it: it searches the
        // tags) has the next chunk's id there, and that is taken as it stands
        if ((size & 1u) && pos < len && file[pos] == 0) pos++;
    }
    if (!have_fmt || !have_data) return MP3S_E_EXIT;
    *msg = "Unsupported WAVE file, compression used instead of PCM.";
    if (fmt_size != 16 && fmt_size != 18 && fmt_size != 40) return MP3S_E_EXIT;
    *msg = "short WAVE header";
    if (fmt_at + fmt_size > len) return MP3S_E_MALFORMED;
    uint32_t tag = 0, ch = 0, rate = 0, bits = 0;
    le(file, len, (long)fmt_at, 2, &tag); le(file, len, (long)fmt_at + 2, 2, &ch);
    le(file, len, (long)fmt_at + 4, 4, &rate); le(file, len, (long)fmt_at + 14, 2, &bits);
    *msg = "Unsupported WAVE file, compression used instead of PCM.";
    if (tag == 0xfffe) {   // WAVE_FORMAT_EXTENSIBLE: the tag is the start of the sub-format GUID, the width is the container's
        if (fmt_size != 40) return MP3S_E_EXIT;
        le(file, len, (long)fmt_at + 24, 2, &tag);
        if (tag == 0xfffe) return MP3S_E_EXIT;
    }
    if (tag != 1 && tag != 3) return MP3S_E_EXIT;
    o->channels = (int32_t)ch; o->samplerate = (int32_t)rate; o->bits_per_sample = (int32_t)bits; o->bitrate = bitrate_kbps;
    *msg = "WAVE header with zero channels (ZeroDivisionError in the reference)";
    if (ch == 0) return MP3S_E_MALFORMED;
    *msg = "more than two channels";
    if (ch > 2) return MP3S_E_UNSUPPORTED;
    *msg = "Unsupported sampling frequency.";
    if (!resample) {
        if (rate != 32000 && rate != 44100 && rate != 48000) return MP3S_E_EXIT;
        out_rate = (int)rate;
    } else if (rate > 0x7fffffffu || wav_resample_plan((int)rate, resample, &out_rate, &rL, &rM, &rT, &rH)) return MP3S_E_EXIT;
    *msg = "Unsupported WAVE file, samples not int8, int16 or int32 type.";
    if (tag == 3) {
        if (bits != 32) return MP3S_E_EXIT;
        o->format = MP3S_WAV_F32;
    } else {
        if (bits != 8 && bits != 16 && bits != 24 && bits != 32) return MP3S_E_EXIT;
        o->format = bits == 8 ? MP3S_WAV_U8 : bits == 16 ? MP3S_WAV_S16 : bits == 24 ? MP3S_WAV_S24 : MP3S_WAV_S32;
    }
    o->block_align = (int32_t)(ch * (bits / 8));   // (computed: the field in the file is not trusted)
    int sri, bri, whole;
    *msg = "Unsupported bitrate configuration.";
    if (stream_params(out_rate, bitrate_kbps, &sri, &bri, &whole)) return MP3S_E_EXIT;
    const uint64_t left = len - data_at;
    const uint64_t bytes = data_size == 0 || data_size == 0xffffffffu || data_size > left ? left : data_size;   // (0 / all ones: to the end of the file)
    o->data_offset = (int64_t)data_at;
    o->n_samples = (int64_t)(bytes / (uint64_t)o->block_align);   // (a cut last sample is dropped)
    o->n_frames = (o->n_samples + 1151) / 1152;
    *msg = "no samples";
    if (o->n_samples == 0) return MP3S_E_UNSUPPORTED;
    *msg = "";
    if (rs) {
        rs->in = *o;
        rs->out_rate = out_rate; rs->L = rL; rs->M = rM; rs->taps = rT; rs->half = rH;
        rs->n_out = (int64_t)(((unsigned __int128)o->n_samples * (unsigned)rL + (unsigned)rM - 1) / (unsigned)rM);
        rs->n_frames = (rs->n_out + 1151) / 1152;
    }
    return MP3S_OK;
}

// The resampler of MP3S_OPT_WAV_RESAMPLE (the rules are stated at mp3s_wav_resample_info in include/mp3s.h), host part: the target
// rate, the ratio and the integer tap table.  Everything the device computes with is an integer made here.
int wav_resample_plan(int in_rate, int mode, int *out_rate, int *L, int *M, int *T, int *H)
{
    static const int kRates[3] = {32000, 44100, 48000};
    if (in_rate <= 0) return 1;
    auto gcd = [](int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; };
    int target = 0;
    if (mode != 1) target = mode;
    else if (in_rate == 32000 || in_rate == 44100 || in_rate == 48000) target = in_rate;
    else {
        // the supported rates not below the file's (all three above 48 000 Hz): the smallest L, then the highest rate
        int64_t best = 0;
        for (int r : kRates) {
            if (in_rate <= 48000 && r < in_rate) continue;
            const int64_t l = r / gcd(r, in_rate);
            if (!target || l <= best) { target = r; best = l; }
        }
    }
    if (pcm_resample_ratio(in_rate, target, L, M, T, H)) return 1;
    *out_rate = target;
    return 0;
}

// the ratio of ANY pair of rates by the same rules (mp3s_pcm_resample_plan: the PCM batch calls that take a rate)
int pcm_resample_ratio(int in_rate, int out_rate, int *L, int *M, int *T, int *H)
{
    if (in_rate <= 0 || out_rate <= 0) return 1;
    auto gcd = [](int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; };
    const int64_t g = gcd(out_rate, in_rate);
    const int64_t l = out_rate / g, m = in_rate / g;
    // rho = min(1, L / M); H = ceil(16 / rho)
    const int64_t h = l >= m ? 16 : (16 * m + l - 1) / l;
    if (l > 1280 || 2 * h > 256) return 1;
    *L = (int)l; *M = (int)m; *H = (int)h; *T = (int)(2 * h);
    return 0;
}

int pcm_resample_plan(int in_rate, int out_rate, int *L, int *M, int *T, int *H)
{
    if (pcm_resample_ratio(in_rate, out_rate, L, M, T, H)) return 1;
    if (*L == 1 && *M == 1) return 0;                  // (not resampled: no table is asked for)
    // the table's own bound (sum |c| of either half of a phase): a ratio is met again and again, so what it gave is kept
    static std::mutex mu;
    static std::map<std::pair<int, int>, bool> known;
    std::lock_guard<std::mutex> lock(mu);
    const auto it = known.find({*L, *M});
    if (it != known.end()) return it->second ? 0 : 1;
    std::vector<int32_t> taps;
    int t = 0;
    const bool ok = wav_resample_taps(*L, *M, taps, &t) == 0 && t == *T;
    known[{*L, *M}] = ok;
    return ok ? 0 : 1;
}

int wav_resample_taps(int L, int M, std::vector<int32_t> &c, int *T_out)
{
    if (L < 1 || M < 1 || L > 1280) return 1;
    const int64_t h64 = L >= M ? 16 : (16 * (int64_t)M + L - 1) / L;
    if (2 * h64 > 256) return 1;
    const int H = (int)h64, T = 2 * H;
    const double pi = 3.14159265358979323846;
    const double rho = L >= M ? 1.0 : (double)L / (double)M, fc = 0.95 * rho;
    c.assign((size_t)L * (size_t)T, 0);
    for (int p = 0; p < L; p++) {
        int32_t *row = c.data() + (size_t)p * (size_t)T;
        int64_t sum = 0;
        int big = 0;
        for (int k = 0; k < T; k++) {
            const double t = (double)(k - H + 1) - (double)p / (double)L;
            const double u = t / (double)H;
            double w = 0.0;
            if (u > -1.0 && u <= 1.0) w = 0.35875 + 0.48829 * cos(pi * u) + 0.14128 * cos(2.0 * pi * u) + 0.01168 * cos(3.0 * pi * u);
            const double x = fc * t;
            const double sinc = x == 0.0 ? 1.0 : sin(pi * x) / (pi * x);
            row[k] = (int32_t)rint(fc * sinc * w * 32768.0);
            sum += row[k];
            if (row[k] > row[big]) big = k;           // (the first of equal taps)
        }
        row[big] += (int32_t)(32768 - sum);            // DC gain exactly 1
        // the bound that keeps the device's sums inside int32: it adds the taps below 2 (H / 2) and the rest apart (65535 x 32768 + 2^14 < 2^31)
        // and joins the two in 64 bits.  (One sum over the phase would not do: sum |c| is 69 292 for L / M = 2 / 1.)
        int64_t mag[2] = {0, 0};
        for (int k = 0; k < T; k++) mag[k >= 2 * (H / 2)] += row[k] < 0 ? -(int64_t)row[k] : row[k];
        if (mag[0] > 65535 || mag[1] > 65535) return 1;
    }
    *T_out = T;
    return 0;
}

// the 44 bytes scipy.io.wavfile.write puts in front of int16 data (reference MP3_Parser.py:86-93 -> scipy)
void wav_header(int64_t n_rows, int nch, int rate, uint8_t *h)
{
    auto put = [&](int at, uint32_t v, int bytes) { for (int i = 0; i < bytes; i++) h[at + i] = (uint8_t)(v >> (8 * i)); };
    const uint32_t nb = (uint32_t)(n_rows * nch * 2);
    memcpy(h, "RIFF", 4); put(4, 36 + nb, 4); memcpy(h + 8, "WAVEfmt ", 8);
    put(16, 16, 4); put(20, 1, 2); put(22, (uint32_t)nch, 2); put(24, (uint32_t)rate, 4);
    put(28, (uint32_t)(rate * nch * 2), 4); put(32, (uint32_t)(nch * 2), 2); put(34, 16, 2);
    memcpy(h + 36, "data", 4); put(40, nb, 4);
}

// reference steganography.py:10-24, 42-50: str(len(message)) + '#' + message, UTF-8, MSB first.  len() counts code
// points while the payload is UTF-8 bytes, so a non-ASCII message reveals truncated -- kept.
void message_frame(const uint8_t *utf8, size_t n, std::vector<uint8_t> &bits)
{
    size_t chars = 0;
    for (size_t i = 0; i < n; i++) chars += (utf8[i] & 0xc0) != 0x80;
    char head[32];
    const int hn = snprintf(head, sizeof head, "%zu#", chars);
    bits.clear();
    bits.reserve((hn + n) * 8);
    auto push = [&](uint8_t b) { for (int k = 7; k >= 0; k--) bits.push_back((b >> k) & 1); };
    for (int i = 0; i < hn; i++) push((uint8_t)head[i]);
    for (size_t i = 0; i < n; i++) push(utf8[i]);
}

// reference decoder/decoder.py:90-108: bytes -> chr() each, digits up to the first '#', int() or 0, slice, UTF-8.
void message_reveal(const uint8_t *bits, size_t n_bits, std::vector<uint8_t> &text)
{
    const size_t n = n_bits / 8;   // zip(*[iter(bits)] * 8) drops an incomplete last byte
    std::vector<uint8_t> s(n);
    for (size_t i = 0; i < n; i++) {
        uint8_t b = 0;
        for (int k = 0; k < 8; k++) b = (uint8_t)((b << 1) | (bits[i * 8 + k] & 1));
        s[i] = b;
    }
    size_t head = 0;
    while (head < n && s[head] != '#') head++;   // no '#': the whole string is the "length"
    int64_t mlen = 0;
    if (!py_int(s.data(), head, &mlen)) { mlen = 0; head = 0; }
    // Python slices: [a:] or [a:a+mlen] with negative ends counted from the back and everything clamped
    const int64_t L = (int64_t)n, a = (int64_t)head + 1;
    int64_t lo = a < L ? a : L, hi = L;
    if (!(a + mlen > L)) {
        hi = a + mlen;
        if (hi < 0) { hi += L; if (hi < 0) hi = 0; }
    }
    text.clear();
    for (int64_t i = lo; i < hi; i++) {   // bytes(str, 'utf-8') of code points below 256
        if (s[i] < 0x80) text.push_back(s[i]);
        else { text.push_back((uint8_t)(0xc0 | (s[i] >> 6))); text.push_back((uint8_t)(0x80 | (s[i] & 0x3f))); }
    }
}

}  // namespace mp3s
