"""Writes tests/golden/tlsh_v1.json: fixed inputs and the digests tests/tlsh_ref.py gives for them, so that the
restatement and the kernel cannot drift together unnoticed.  The inputs are stored with the digests (hex).

    python tools/gen_tlsh_golden.py
"""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tlsh_ref  # noqa: E402

WORDS = ("the of and a to in is you that it he was for on are as with his they I at be this have from or one had by word "
         "but not what all were we when your can said there use an each which she do how their if will up other about out "
         "many then them these so some her would make like him into time has look two more write go see number no way could "
         "people my than first water been call who oil its now find long down day did get come made may part").split()


def prose(seed: int, n_words: int) -> bytes:
    rng = random.Random(seed)
    return " ".join(rng.choice(WORDS) for _ in range(n_words)).encode()


def cases():
    pangram = b"The quick brown fox jumps over the lazy dog. "
    rb = random.Random(99)
    return [
        ("pangram_x2", pangram * 2),
        ("pangram_x40", pangram * 40),
        ("all_bytes_x2", bytes(range(256)) * 2),
        ("prose_60_words", prose(1, 60)),
        ("prose_700_words", prose(2, 700)),
        ("prose_700_words_edited", prose(2, 700).replace(b" the ", b" THE ", 3)),
        ("random_bytes_50", bytes(rb.randrange(256) for _ in range(50))),
        ("random_bytes_657", bytes(rb.randrange(256) for _ in range(657))),
        ("random_bytes_3200", bytes(rb.randrange(256) for _ in range(3200))),
        ("zeros_then_prose", b"\0" * 64 + prose(3, 80) + b"\0"),
        ("refused_64_buckets", b"acabacbaacacababaaccbcabccababcbcabcacabacacaaacbaaaaccbbbaaabcbcabcbaaca"),
    ]


def main():
    out = []
    for name, data in cases():
        d = tlsh_ref.digest(data)
        out.append({"name": name, "input_hex": data.hex(), "digest": tlsh_ref.hexdigest(d) if d is not None else None})
    path = os.path.join(ROOT, "tests", "golden", "tlsh_v1.json")
    with open(path, "w") as f:
        json.dump({"algorithm": "tlsh-128-1", "source": "tests/tlsh_ref.py", "cases": out}, f, indent=1)
        f.write("\n")
    print("wrote", path, len(out), "cases")


if __name__ == "__main__":
    main()
