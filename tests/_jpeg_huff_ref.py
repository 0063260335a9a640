"""Python restatement of the device Huffman decoder of csrc/jpeg_huff.hip: the host staging of the scan (wu_jpeg_scan_stage) and the
self-synchronising walk (rounds, carry, count, write, DC scan, magnitude).  Written from the description of the algorithm, with plain
Python integers and dictionaries; it shares no code with the library.  Headers come from wu.jpeg.parse (the marker walk is not what is
restated here).  Test infrastructure, like _jpeg_ref.py.

A state is (p, b, k): bit position in the image's staged scan, block-in-MCU, zig-zag index of the next coefficient (0 = DC next).
"""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
BAD_CODE, DC_CATEGORY, INDEX, SHORT, DC_RANGE, MAGNITUDE = 0x100, 0x200, 0x400, 0x800, 0x1000, 11
MAX_BLOCK_L1 = 5900
CHUNK = 256


class StageError(ValueError):
    def __init__(self, code, what):
        super().__init__(what)
        self.code = code


def count_values(counts):
    code = k = 0
    for l in range(1, 17):
        c = counts[l - 1]
        if code + c > (1 << l):
            return -1
        k += c
        code = (code + c) << 1
    return k if k <= 256 else -1


def n_segments(info):
    mcus = info.mcus_x * info.mcus_y
    return -(-mcus // info.restart_interval) if info.restart_interval > 0 else 1


def scan_stage(data, info, S):
    """The staged form of a parsed file: dict(scan bytes, segs [(first_subseq, bit_length, first_mcu, mcu_count)], dht (1632 bytes),
    qtab (3, 64) uint16 natural order, n_subseq)."""
    n = len(data)
    dht = bytearray(6 * 272)
    qtab = np.ones((3, 64), np.uint16)
    for c in range(info.ncomp):
        od, oa, oq = info.dht_off[info.td[c]], info.dht_off[4 + info.ta[c]], info.dqt_off[info.tq[c]]
        nd, na = count_values(data[od:od + 16]), count_values(data[oa:oa + 16])
        if nd < 0 or na < 0 or od + 16 + nd > n or oa + 16 + na > n:
            raise StageError(-2, "corrupt Huffman table")
        dht[c * 272:c * 272 + 16 + nd] = data[od:od + 16 + nd]
        dht[(3 + c) * 272:(3 + c) * 272 + 16 + na] = data[oa:oa + 16 + na]
        for k in range(64):
            qtab[c, ZIGZAG[k]] = data[oq + k]
    sub = S // 8
    mcus, ri = info.mcus_x * info.mcus_y, info.restart_interval
    out, segs = bytearray(), []
    pos, next_rst, nseg = info.scan_offset, 0, n_segments(info)
    for s in range(nseg):
        start = len(out)
        while pos < n:
            b = data[pos]
            if b != 0xFF:
                out.append(b)
                pos += 1
            elif pos + 1 < n and data[pos + 1] == 0:
                out.append(0xFF)
                pos += 2
            else:
                break
        length = len(out) - start
        nsub = max(1, -(-length // sub))
        out.extend(bytes(start + nsub * sub - len(out)))
        segs.append((start // sub, length * 8, s * ri if ri else 0, min(ri, mcus - s * ri) if ri else mcus))
        if s + 1 < nseg:
            if pos + 1 >= n or data[pos] != 0xFF or data[pos + 1] != 0xD0 + next_rst:
                raise StageError(-3, f"bad restart marker sequence at MCU {(s + 1) * ri}")
            pos += 2
            next_rst = (next_rst + 1) & 7
    n_subseq = len(out) // sub
    out.extend(bytes(-(len(out) + 8) % 16 + 8))
    return dict(scan=bytes(out), segs=segs, dht=bytes(dht), qtab=qtab, n_subseq=n_subseq)


class Table:
    """Canonical Huffman code of 16 counts + values: {(length, code): symbol}."""
    def __init__(self, raw):
        self.codes = {}
        code = k = 0
        for l in range(1, 17):
            for _ in range(raw[l - 1]):
                self.codes[(l, code)] = raw[16 + k]
                code += 1
                k += 1
            code <<= 1
        self.cache = {}

    def symbol(self, w16):
        """(symbol or -1, bits consumed) for the 16 bits w16 (MSB first)."""
        hit = self.cache.get(w16)
        if hit is None:
            hit = (-1, 16)
            for l in range(1, 17):
                sym = self.codes.get((l, w16 >> (16 - l)))
                if sym is not None:
                    hit = (sym, l)
                    break
            self.cache[w16] = hit
        return hit


def extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


class Walker:
    def __init__(self, stage, info, S):
        self.S = S
        self.scan = stage["scan"]
        self.big = int.from_bytes(self.scan + bytes(8), "big")
        self.nbits = (len(self.scan) + 8) * 8
        self.region_bits = len(self.scan) * 8
        self.segs = stage["segs"]
        self.nsub = stage["n_subseq"]
        self.tables = [Table(stage["dht"][t * 272:(t + 1) * 272]) for t in range(6)]
        self.hs0, self.vs0, self.ncomp = info.hs[0], info.vs[0], info.ncomp
        self.hv = self.hs0 * self.vs0
        self.bpm = self.hv + (2 if info.ncomp == 3 else 0)
        self.mcus_x, self.total_mcus = info.mcus_x, info.mcus_x * info.mcus_y
        self.nblocks = info.total_blocks
        self.ri = info.restart_interval
        self.memo = {}
        self.rounds = []          # per chunk: the last round in which a state was overwritten
        self.exits = None         # decode() keeps the walk's exit states here

    def peek32(self, p):
        if p >= self.region_bits:
            return 0
        return (self.big >> (self.nbits - p - 32)) & 0xFFFFFFFF

    def step(self, st):
        """One symbol: (state', error bits, zig-zag index or -1, value)."""
        p, b, k = st
        comp = 0 if b < self.hv else 1 + b - self.hv
        w = self.peek32(p)
        err, out_k, out_v = 0, -1, 0
        if k == 0:
            sym, ln = self.tables[comp].symbol(w >> 16)
            if sym < 0:
                err, sym = BAD_CODE, 0
            elif sym > 15:
                err, sym = DC_CATEGORY, sym & 15
            if sym:
                out_v = extend(((w << ln) & 0xFFFFFFFF) >> (32 - sym), sym)
            out_k, p, k = 0, p + ln + sym, 1
        else:
            rs, ln = self.tables[3 + comp].symbol(w >> 16)
            if rs < 0:
                err, rs = BAD_CODE, 0
            r, sz = rs >> 4, rs & 15
            if sz == 0:
                k = k + 16 if r == 15 else 64
                p += ln
            else:
                k += r
                if k > 63:
                    err, k = INDEX, 63
                else:
                    out_k, out_v = k, extend(((w << ln) & 0xFFFFFFFF) >> (32 - sz), sz)
                k += 1
                p += ln + sz
        if k >= 64:
            k, b = 0, (b + 1) % self.bpm
        return (p, b, k), err, out_k, out_v

    def run(self, st, end):
        """Exit state of decoding the symbols that start in front of bit `end`; memoised, the function is pure."""
        key = (st, end)
        hit = self.memo.get(key)
        if hit is None:
            cur = st
            while cur[0] < end:
                cur = self.step(cur)[0]
            hit = self.memo[key] = cur
        return hit

    def segment_of(self, g):
        sj = 0
        for j, sg in enumerate(self.segs):
            if sg[0] <= g:
                sj = j
        return sj

    def block_index(self, m0, o):
        mcu, bi = m0 + o // self.bpm, o % self.bpm
        my, mx = divmod(mcu, self.mcus_x)
        if bi < self.hv:
            return (my * self.vs0 + bi // self.hs0) * (self.mcus_x * self.hs0) + mx * self.hs0 + bi % self.hs0
        return self.total_mcus * self.hv + (bi - self.hv) * self.total_mcus + mcu

    def walk(self):
        """(coefficients with DC differences (nblocks, 64) int32, status, exit states of every subsequence)."""
        S = self.S
        coef = np.zeros((self.nblocks, 64), np.int32)
        status = 0
        seg_first = [sg[0] for sg in self.segs]
        seg_of, j = [], 0
        for g in range(self.nsub):
            while j + 1 < len(self.segs) and seg_first[j + 1] <= g:
                j += 1
            seg_of.append(j)
        carry_state, carry_blocks = (0, 0, 0), 0
        exits = []
        for c0 in range(0, self.nsub, CHUNK):
            nt = min(CHUNK, self.nsub - c0)
            seg_end = [seg_first[seg_of[c0 + i] + 1] if seg_of[c0 + i] + 1 < len(self.segs) else self.nsub for i in range(nt)]
            exact = [c0 + i == seg_first[seg_of[c0 + i]] or i == 0 for i in range(nt)]
            entry = [((c0 + i) * S, 0, 0) for i in range(nt)]
            if c0 != seg_first[seg_of[c0]]:
                entry[0] = carry_state
            st = [self.run(entry[i], (c0 + i + 1) * S) for i in range(nt)]
            e = list(st)
            active = [True] * nt
            rounds = 0
            for r in range(1, CHUNK):
                writes = []
                for i in range(nt):
                    j = i + r
                    if active[i] and (j >= CHUNK or c0 + j >= seg_end[i]):
                        active[i] = False
                    if active[i]:
                        st[i] = self.run(st[i], (c0 + j + 1) * S)
                        if st[i] == e[j]:
                            active[i] = False
                        else:
                            writes.append((j, st[i]))
                for j, v in writes:           # after every comparison of the round, as behind the barrier
                    e[j] = v
                if not writes:
                    break
                rounds = r
            self.rounds.append(rounds)
            exits.extend(e)
            for i in range(1, nt):
                if not exact[i]:
                    entry[i] = e[i - 1]
            # count
            begun = []
            for i in range(nt):
                cur, n = entry[i], 0
                while cur[0] < (c0 + i + 1) * S:
                    n += cur[2] == 0
                    cur = self.step(cur)[0]
                begun.append(n)
            excl = [0] * nt
            for i in range(1, nt):
                excl[i] = excl[i - 1] + begun[i - 1]
            first = []
            for i in range(nt):
                ss = seg_first[seg_of[c0 + i]]
                first.append(excl[i] - excl[ss - c0] if ss >= c0 else carry_blocks + excl[i])
            # write
            for i in range(nt):
                g = c0 + i
                ss, seg_bits, m0, mc = self.segs[seg_of[g]]
                total, end, seg_end_bit = mc * self.bpm, (g + 1) * S, ss * S + seg_bits
                last_seg = seg_of[g] + 1 == len(self.segs)
                cur, nxt = entry[i], first[i]
                blk, in_block, err = None, False, 0
                if cur[2] != 0 and 1 <= nxt <= total:
                    in_block, blk = True, self.block_index(m0, nxt - 1)
                while cur[0] < end:
                    if cur[2] == 0:
                        if nxt >= total:
                            in_block = False
                            break
                        blk, in_block = self.block_index(m0, nxt), True
                        nxt += 1
                    cur, e1, k, v = self.step(cur)
                    if in_block:
                        err |= e1
                        if cur[0] > seg_end_bit:
                            err |= SHORT
                        elif k >= 0 and 0 <= blk < self.nblocks:
                            coef[blk, ZIGZAG[k]] = v
                        if cur[2] == 0 and nxt == total and not last_seg and cur[0] <= seg_end_bit and seg_end_bit - cur[0] >= 64:
                            err |= SHORT
                if g == seg_end[i] - 1 and (nxt < total or (in_block and cur[2] != 0)):
                    err |= SHORT
                status |= err
            if nt == CHUNK:
                ss = seg_first[seg_of[c0 + CHUNK - 1]]
                carry_state, carry_blocks = e[CHUNK - 1], first[CHUNK - 1] + begun[CHUNK - 1]
        return coef, status, exits

    def dc_and_magnitude(self, coef, qtab):
        """DC differences -> values in place per (component, segment) in scan order; returns the status bits."""
        status = 0
        for c in range(self.ncomp):
            hs, vs = (self.hs0, self.vs0) if c == 0 else (1, 1)
            plane = 0 if c == 0 else self.total_mcus * self.hv + (c - 1) * self.total_mcus
            pred = 0
            for mcu in range(self.total_mcus):
                if (mcu % self.ri == 0) if self.ri else mcu == 0:
                    pred = 0
                my, mx = divmod(mcu, self.mcus_x)
                for v in range(vs):
                    for h in range(hs):
                        b = plane + (my * vs + v) * (self.mcus_x * hs) + mx * hs + h
                        pred += int(coef[b, 0])
                        if not -32768 <= pred <= 32767:
                            status |= DC_RANGE
                        coef[b, 0] = ((pred + 32768) & 0xFFFF) - 32768
            blocks = coef[plane:plane + self.total_mcus * hs * vs]
            if blocks.size and int((np.abs(blocks) * qtab[c].astype(np.int64)).sum(1).max()) > MAX_BLOCK_L1:
                status |= MAGNITUDE
        return status


def sequential_exits(w):
    """Exit state of every subsequence by ONE sequential decode per segment: what the walk has to reproduce."""
    out = []
    for j, (ss, _, _, _) in enumerate(w.segs):
        se = w.segs[j + 1][0] if j + 1 < len(w.segs) else w.nsub
        st = (ss * w.S, 0, 0)
        for g in range(ss, se):
            st = w.run(st, (g + 1) * w.S)
            out.append(st)
    return out


def decode(data, info, S):
    """(coef (nblocks, 64) int16, qtab (3, 64) uint16, status, Walker) of a parsed file through stage + walk + DC scan."""
    stage = scan_stage(data, info, S)
    w = Walker(stage, info, S)
    coef, status, w.exits = w.walk()
    status |= w.dc_and_magnitude(coef, stage["qtab"])
    return coef.astype(np.int16), stage["qtab"], status, w
