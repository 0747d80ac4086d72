"""Morse code beside the CW decoder bank (cw.py, include/ka9q_hip.h: kq_cw_*), plain Python: the alphabet as data, the
bank's geometry for a top speed, keyed audio for test traffic and the reader of the bank's events.

A character's code is its elements behind a leading 1, the first element in the highest place, a dot 0 and a dash 1: E is
0b10, T 0b11, A (.-) 0b101.  Code 1 (no element) is a word gap and code 0 a character the decoder could not take.
"""
import numpy as np

LETTERS = {
    "A": ".-", "B": "-...", "C": "-.-.", "D": "-..", "E": ".", "F": "..-.", "G": "--.", "H": "....", "I": "..", "J": ".---",
    "K": "-.-", "L": ".-..", "M": "--", "N": "-.", "O": "---", "P": ".--.", "Q": "--.-", "R": ".-.", "S": "...", "T": "-",
    "U": "..-", "V": "...-", "W": ".--", "X": "-..-", "Y": "-.--", "Z": "--..",
}
DIGITS = {"0": "-----", "1": ".----", "2": "..---", "3": "...--", "4": "....-", "5": ".....", "6": "-....", "7": "--...",
          "8": "---..", "9": "----."}
# "=", "+" and "(" are left to the prosigns BT, AR and KN, which are keyed alike
PUNCTUATION = {".": ".-.-.-", ",": "--..--", "?": "..--..", "/": "-..-.", "'": ".----.", "!": "-.-.--", ")": "-.--.-",
               "&": ".-...", ":": "---...", ";": "-.-.-.", "-": "-....-", "_": "..--.-", '"': ".-..-.", "$": "...-..-",
               "@": ".--.-."}
PROSIGNS = {"AR": ".-.-.", "SK": "...-.-", "BT": "-...-", "KN": "-.--."}     # written <AR> in a text

WORD_GAP, UNDECODABLE = 1, 0


def code_of(elements):
    """".-" -> 0b101"""
    c = 1
    for e in elements:
        c = 2 * c + (e == "-")
    return c


def elements_of(code):
    """0b101 -> ".-" (codes 0 and 1: "")"""
    return "".join(".-"[int(b)] for b in bin(code)[3:]) if code > 1 else ""


ALPHABET = {k: code_of(v) for k, v in {**LETTERS, **DIGITS, **PUNCTUATION}.items()}
ALPHABET.update({"<%s>" % k: code_of(v) for k, v in PROSIGNS.items()})
CHARACTERS = {v: k for k, v in ALPHABET.items()}
assert len(CHARACTERS) == len(ALPHABET)


def unit_of(fs, block_len, wpm):
    """the dot of `wpm` words per minute (1.2 / wpm seconds, the word PARIS) in sixteenths of a frame, a double"""
    return 19.2 * float(fs) / (float(block_len) * float(wpm))


def cw_config(fs, max_wpm=60.0, min_wpm=5.0):
    """CwBank keywords for a top speed: the longest frame that leaves a dot of max_wpm at least 4 frames (at most 4096
    samples): 60 at 12 kHz and 60 WPM, where a dot is 20 ms"""
    block_len = int(min(4096, 0.3 * float(fs) / float(max_wpm) + 1e-9))
    if block_len < 8:
        raise ValueError("%g Hz is too slow for %g WPM" % (fs, max_wpm))
    return dict(block_len=block_len, min_wpm=float(min_wpm), max_wpm=float(max_wpm))


def _tokens(text):
    """the characters of a text, prosigns in <> as one; a run of blanks is one " \""""
    out, i, text = [], 0, " ".join(text.upper().split())
    while i < len(text):
        j = text.find(">", i) + 1 if text[i] == "<" else i + 1
        if j <= i:
            raise ValueError("unclosed < in %r" % text)
        out.append(text[i:j])
        i = j
    return out


def keying(text):
    """the text as (mark?, dots) pairs: dot 1, dash 3, between elements 1, between characters 3, between words 7"""
    out = []
    for tok in _tokens(text):
        if tok == " ":
            if out:
                out[-1] = (False, 7)
            continue
        if tok not in ALPHABET:
            raise ValueError("no Morse for %r" % tok)
        for e in elements_of(ALPHABET[tok]):
            out += [(True, 3 if e == "-" else 1), (False, 1)]
        out[-1] = (False, 3)
    return out


def encode(text, wpm, fs, pitch=700.0, amp=0.3, rise_ms=5.0, lead=0.0, tail=None):
    """Keyed audio, float32: a tone of `pitch` Hz and amplitude `amp` keyed with `text` at `wpm` (a dot is 1.2 / wpm
    seconds), the edges raised cosines of rise_ms centred on the keying instants; `lead` seconds of silence ahead and
    `tail` behind (default: 10 dots, so that a decoder closes the last character and files the word gap)."""
    fs = float(fs)
    dot = 1.2 / float(wpm)
    if tail is None:
        tail = 10 * dot
    t, edges = float(lead), []
    for mark, dots in keying(text):
        if mark:
            edges.append((t, t + dots * dot))
        t += dots * dot
    n = int(round((t + tail) * fs))
    at = np.arange(n) / fs
    r = max(rise_ms * 1e-3, 1e-9)
    env = np.zeros(n)
    for a, b in edges:
        i0, i1 = max(0, int((a - r) * fs)), min(n, int((b + r) * fs) + 2)
        tt = at[i0:i1]
        up = np.clip((tt - a) / r + 0.5, 0.0, 1.0)
        down = np.clip((b - tt) / r + 0.5, 0.0, 1.0)
        env[i0:i1] += 0.5 * (1.0 - np.cos(np.pi * np.minimum(up, down)))
    return (amp * env * np.sin(2.0 * np.pi * pitch * at)).astype(np.float32)


def read_text(events):
    """the events of one slot (anything with a `code`) as text: a character per code, a word gap as one blank, what has
    no character as "?"; leading and trailing blanks go"""
    out = []
    for e in events:
        c = int(e.code)
        if c == WORD_GAP:
            if out and out[-1] != " ":
                out.append(" ")
        else:
            out.append(CHARACTERS.get(c, "?"))
    return "".join(out).strip()


__all__ = ["LETTERS", "DIGITS", "PUNCTUATION", "PROSIGNS", "ALPHABET", "CHARACTERS", "WORD_GAP", "UNDECODABLE", "code_of",
           "elements_of", "unit_of", "cw_config", "keying", "encode", "read_text"]
