"""Types shared by the effects.  Reference: ``src/torchfx/typing.py`` -- only ``MusicalTime`` (:50-158), the note value a
BPM-synced ``Delay`` is given in, is needed here."""
from __future__ import annotations

import re
from dataclasses import dataclass

_MUSICAL_TIME = re.compile(r"(\d+)/(\d+)([dt]?)$")
_MODIFIER_FACTOR = {"": 1.0, "d": 1.5, "t": 1 / 3}      # plain, dotted, triplet


@dataclass(frozen=True)
class MusicalTime:
    """A note value as a fraction of a bar: ``numerator / denominator``, optionally dotted (``"d"``, x 1.5) or a triplet
    (``"t"``, x 1/3).  ``"1/4"`` is a quarter of a bar in any time signature; the bar's length comes from the tempo."""

    numerator: int
    denominator: int
    modifier: str = ""

    def fraction(self) -> float:
        """The note's length in bars.  Raises ``ValueError`` for a modifier other than "", "d" or "t"."""
        factor = _MODIFIER_FACTOR.get(self.modifier)
        if factor is None:
            raise ValueError(f"Invalid time duration modifier: {self.modifier}")
        return self.numerator / self.denominator * factor

    def duration_seconds(self, bpm: float, beats_per_bar: int = 4) -> float:
        """The note's length in seconds at ``bpm`` beats per minute and ``beats_per_bar`` beats in a bar."""
        assert bpm > 0, "BPM must be positive"
        return self.fraction() * (60.0 / bpm * beats_per_bar)

    @classmethod
    def from_string(cls, s: str) -> "MusicalTime":
        """Parse ``"n/d"`` with an optional ``d`` / ``t`` suffix (``"1/8"``, ``"1/4d"``, ``"1/8t"``)."""
        m = _MUSICAL_TIME.match(s)
        if m is None:
            raise ValueError(f"Invalid musical time string: {s}")
        return cls(int(m.group(1)), int(m.group(2)), m.group(3))
