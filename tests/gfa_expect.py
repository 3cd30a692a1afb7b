"""A pure-Python reader of the GFA subset a construction accepts (include/gbwt_hip.h, "construction from GFA"), written from that contract
and not from the library: what a built handle must hold.  Refusals are exceptions that carry the 1-based line number."""
import re


class Refused(Exception):
    def __init__(self, line, status, what):
        super().__init__(f"line {line}: {what}")
        self.line, self.status = line, status


INVALID_DATA, UNSUPPORTED = "INVALID_DATA", "UNSUPPORTED"


def _node_id(token):
    return token.isdigit() and token.isascii() and len(token) <= 10 and token[0] != "0" and 1 <= int(token) <= 2**31 - 1


class Expected:
    """paths: rows of GBWT nodes (2 * id + reverse) in path order -- the P-lines, then the W-lines; names: (sample, contig, phase, fragment)
    per path as ids; samples / contigs: the name lists; labels: {node id: sequence} of every S-line; visited: the node ids on a path."""

    def __init__(self, text):
        if isinstance(text, str):
            text = text.encode()
        errors = []                                    # (line, status, what): the first in file order is raised
        segments, p_lines, w_lines = {}, [], []
        self.reference_samples = None
        self.ignored = self.links = 0
        lines = text.split(b"\n")
        if lines and lines[-1] == b"":
            lines.pop()
        for number, raw in enumerate(lines, 1):
            if b"\r" in raw:
                errors.append((number, INVALID_DATA, "carriage return"))
                continue
            if not raw:
                continue
            f = raw.decode("latin-1").split("\t")
            kind = f[0][:1]
            if kind == "" or kind not in "HSLPW":
                self.ignored += 1
            elif kind == "H":
                for field in f[1:]:
                    if field.startswith("RS:Z:") and self.reference_samples is None:
                        self.reference_samples = field[5:]
            elif f[0] != kind or len(f) < {"S": 3, "L": 5, "P": 3, "W": 7}[kind]:
                errors.append((number, INVALID_DATA, "too few fields"))
            elif kind == "S":
                if not _node_id(f[1]):
                    errors.append((number, UNSUPPORTED, "segment name"))
                elif f[2] in ("", "*"):
                    errors.append((number, INVALID_DATA, "no sequence"))
                elif int(f[1]) in segments:
                    errors.append((number, INVALID_DATA, "duplicate segment"))
                else:
                    segments[int(f[1])] = f[2]
            elif kind == "L":
                self.links += 1
            elif kind == "P":
                p_lines.append((number, f))
            else:
                w_lines.append((number, f))
        self.labels = segments
        self.samples = ["_gbwt_ref"] if p_lines else []
        self.contigs, self.paths, self.names, self.path_lines = [], [], [], []
        seen, haplotypes = {}, set()

        def intern(names, s):
            if s not in names:
                names.append(s)
            return names.index(s)

        def steps(number, tokens, walk):
            row = []
            for t in tokens:
                ident, reverse = (t[1:], t[:1] == "<") if walk else (t[:-1], t[-1:] == "-")
                if (t[:1] not in "<>" if walk else t[-1:] not in "+-") or not t or not _node_id(ident):
                    errors.append((number, INVALID_DATA, f"step {t!r}"))
                    return None
                if int(ident) not in segments:
                    errors.append((number, INVALID_DATA, f"unknown segment {ident}"))
                    return None
                row.append(2 * int(ident) + int(reverse))
            return row

        for number, f in p_lines + w_lines:
            walk = f[0] == "W"
            if walk:
                field = "" if f[6] == "*" else f[6]
                tokens = re.findall(r"[<>][^<>]*", field)
                if "".join(tokens) != field:                       # a walk that does not start with a mark
                    tokens = [field]
            else:
                tokens = [] if f[2] in ("", "*") else f[2].split(",")
            row = steps(number, tokens, walk)
            if walk:
                if not (f[2].isdigit() and f[2].isascii() and int(f[2]) < 2**32 - 1):
                    errors.append((number, INVALID_DATA, "haplotype"))
                    continue
                if f[4] != "*" and not (f[4].isdigit() and f[4].isascii() and int(f[4]) < 2**32):
                    errors.append((number, INVALID_DATA, "start"))
                    continue
                name = (intern(self.samples, f[1]), intern(self.contigs, f[3]), int(f[2]), 0 if f[4] == "*" else int(f[4]))
            else:
                name = (0, intern(self.contigs, f[1]), 0, 0)
            if name in seen:
                errors.append((max(number, seen[name]), INVALID_DATA, "duplicate path name"))
            seen.setdefault(name, number)
            haplotypes.add((name[0], name[2]))
            self.paths.append(row)
            self.names.append(name)
            self.path_lines.append(number)
        self.haplotypes = len(haplotypes)
        if errors:
            raise Refused(*min(errors))
        self.visited = sorted({v // 2 for row in self.paths for v in row})
        self.steps = sum(len(row) for row in self.paths)

    def potential_labels(self):
        """The label of every potential node of the GBZ: ids min .. max of the visited ones, b"" where no path goes."""
        if not self.visited:
            return {}
        return {v: (self.labels[v].encode("latin-1") if v in set(self.visited) else b"") for v in range(self.visited[0], self.visited[-1] + 1)}
