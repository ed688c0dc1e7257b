"""types.StrToInt of the reference restated in Python, string for string (no GPU, no libtsq): the expected values of the string arm
of toBool (expression/expression.go:281-326) in the filter tests.  Every function names the reference lines it restates.

str_to_int(b, str_ctx) -> (value, flags): `b` is the cell's bytes, str_ctx the TSQ_STRCTX_* bits of tsq_expr_prog.str_ctx, flags the
TSQ_S2I_* bits of csrc/tsq_device.h (warnings appended, the error returned)."""

NOT_STRICT, TRUNCATE_ERROR, IGNORE_TRUNCATE, EMPTY_NOT_ZERO = 1, 2, 4, 8
TRUNC_WARN, OVF_WARN, ERR_OVF, ERR_TRUNC = 1, 2, 4, 8

# the StatementContext flags ResetContextOfStmt sets (executor/executor.go:609-680) as str_ctx, with the default (strict) SQL mode
CTX_SELECT = 0                                          # CastStrToIntStrict, TruncateAsWarning, InSelectStmt
CTX_DELETE = NOT_STRICT | TRUNCATE_ERROR                # InDeleteStmt, strict mode: truncation is an error
CTX_INSERT = NOT_STRICT | TRUNCATE_ERROR | EMPTY_NOT_ZERO
CTX_OTHER_LOOSE = NOT_STRICT | EMPTY_NOT_ZERO           # e.g. a non-strict-mode UPDATE: truncation is a warning
CTX_IGNORE = NOT_STRICT | IGNORE_TRUNCATE | EMPTY_NOT_ZERO
ALL_CTX = (CTX_SELECT, CTX_DELETE, CTX_INSERT, CTX_OTHER_LOOSE, CTX_IGNORE, TRUNCATE_ERROR, IGNORE_TRUNCATE, NOT_STRICT)

MAX_I64, MIN_I64, MAX_U64 = (1 << 63) - 1, -(1 << 63), (1 << 64) - 1


class GoError(Exception):
    pass


class _Ctx:
    def __init__(self, str_ctx):
        self.flags = str_ctx
        self.warn = 0

    def append_warning(self, kind):  # sc.AppendWarning (stmtctx.go:281-287)
        self.warn |= kind


# ---------------------------------------------------------------- strings.TrimSpace / unicode.IsSpace / utf8
_WHITE_SPACE = {0x9, 0xA, 0xB, 0xC, 0xD, 0x20, 0x85, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000} | set(range(0x2000, 0x200B))


def _decode_rune(b, i):
    """utf8.DecodeRune(b[i:]) -> (rune, size); invalid -> (0xFFFD, 1) (unicode/utf8/utf8.go)."""
    c = b[i]
    if c < 0x80:
        return c, 1
    n = len(b) - i
    if 0xC2 <= c <= 0xDF:
        size, lo, hi = 2, 0x80, 0xBF
    elif 0xE0 <= c <= 0xEF:
        size = 3
        lo, hi = (0xA0, 0xBF) if c == 0xE0 else ((0x80, 0x9F) if c == 0xED else (0x80, 0xBF))
    elif 0xF0 <= c <= 0xF4:
        size = 4
        lo, hi = (0x90, 0xBF) if c == 0xF0 else ((0x80, 0x8F) if c == 0xF4 else (0x80, 0xBF))
    else:
        return 0xFFFD, 1
    if n < size or not (lo <= b[i + 1] <= hi):
        return 0xFFFD, 1
    for k in range(2, size):
        if not (0x80 <= b[i + k] <= 0xBF):
            return 0xFFFD, 1
    r = c & (0x1F if size == 2 else (0x0F if size == 3 else 0x07))
    for k in range(1, size):
        r = (r << 6) | (b[i + k] & 0x3F)
    return r, size


def _decode_last_rune(b):
    """utf8.DecodeLastRune(b) -> (rune, size)."""
    end = len(b)
    if b[end - 1] < 0x80:
        return b[end - 1], 1
    lim = max(end - 4, 0)
    start = end - 1
    while start >= lim:
        if b[start] & 0xC0 != 0x80:  # utf8.RuneStart
            break
        start -= 1
    if start < 0:
        start = 0
    r, size = _decode_rune(b, start)
    if start + size != end:
        return 0xFFFD, 1
    return r, size


def trim_space(b):
    """strings.TrimSpace = TrimFunc(s, unicode.IsSpace) (strings/strings.go)."""
    i = 0
    while i < len(b):
        r, size = _decode_rune(b, i)
        if r not in _WHITE_SPACE:
            break
        i += size
    b = b[i:]
    while b:
        r, size = _decode_last_rune(b)
        if r not in _WHITE_SPACE:
            break
        b = b[:-size]
    return b


# ---------------------------------------------------------------- strconv
def parse_int(s):
    """strconv.ParseInt(s, 10, 64) -> (value, err) with err None / 'syntax' / 'range' (strconv/atoi.go)."""
    if s == "":
        return 0, "syntax"
    neg = False
    body = s
    if s[0] in "+-":
        neg = s[0] == "-"
        body = s[1:]
    # ParseUint(body, 10, 64)
    if body == "":
        return 0, "syntax"
    cutoff = MAX_U64 // 10 + 1
    n = 0
    for c in body:
        if not ("0" <= c <= "9"):
            return 0, "syntax"
        if n >= cutoff:
            n, err = MAX_U64, "range"
            break
        n1 = n * 10 + (ord(c) - 48)
        if n1 > MAX_U64:
            n, err = MAX_U64, "range"
            break
        n = n1
    else:
        err = None
    if not neg and n >= 1 << 63:
        return MAX_I64, "range"
    if neg and n > 1 << 63:
        return MIN_I64, "range"
    if err:
        return (MIN_I64 if neg else MAX_I64), err
    return (-n if neg else n), None


def atoi(s):
    """strconv.Atoi on a 64-bit platform: ParseInt(s, 10, 0) (the fast path gives the same answers)."""
    return parse_int(s)


# ---------------------------------------------------------------- types/convert.go
def _handle_truncate_error(sc):
    """handleTruncateError (types/datum.go:948-957): None, or the error that is returned."""
    if sc.flags & IGNORE_TRUNCATE:
        return None
    if sc.flags & TRUNCATE_ERROR:
        return ERR_TRUNC
    sc.append_warning(TRUNC_WARN)
    return None


def _is_digit(c):
    return "0" <= c <= "9"


def round_int_str(num_next_dot, int_str):
    """roundIntStr (convert.go:284-310).  Raises IndexError where the Go code indexes past a one-character string."""
    if num_next_dot < "5":
        return int_str
    ret = list(int_str)
    idx = len(int_str) - 1
    while idx >= 1:
        if ret[idx] != "9":
            ret[idx] = chr(ord(ret[idx]) + 1)
            break
        ret[idx] = "0"
        idx -= 1
    if idx == 0:
        if int_str[0] == "9":
            ret[0] = "1"
            ret.append("0")
        elif _is_digit(int_str[0]):
            ret[0] = chr(ord(ret[0]) + 1)
        else:
            ret[1] = "1"  # IndexError for a one-character string, as Go panics
            ret.append("0")
    return "".join(ret)


def float_str_to_int_str(sc, valid_float):
    """floatStrToIntStr (convert.go:318-403) -> (int_str, err)."""
    dot_idx = e_idx = -1
    for i, c in enumerate(valid_float):
        if c == ".":
            dot_idx = i
        elif c in "eE":
            e_idx = i
    if e_idx == -1:
        if dot_idx == -1:
            return valid_float, None
        if valid_float[0] in "+-":
            dot_idx -= 1
            digits = valid_float[1:]
        else:
            digits = valid_float
        int_str = "0" if dot_idx == 0 else digits[:dot_idx]
        if len(digits) > dot_idx + 1:
            int_str = round_int_str(digits[dot_idx + 1], int_str)
        if (len(int_str) > 1 or int_str[0] != "0") and valid_float[0] == "-":
            int_str = "-" + int_str
        return int_str, None
    if dot_idx == -1:
        digits = valid_float[:e_idx]
        int_cnt = len(digits)
    else:
        digits = valid_float[:dot_idx]
        int_cnt = len(digits)
        digits += valid_float[dot_idx + 1:e_idx]
    exp, err = atoi(valid_float[e_idx + 1:])
    if err:
        return valid_float, "atoi"
    int_cnt += exp
    if int_cnt > MAX_I64:  # Go's int addition wraps
        int_cnt -= 1 << 64
    if exp >= 0 and (int_cnt > 21 or int_cnt < 0):
        sc.append_warning(OVF_WARN)
        return valid_float[:e_idx], None
    if int_cnt <= 0:
        int_str = "0"
        if int_cnt == 0 and len(digits) > 0 and _is_digit(digits[0]):
            int_str = round_int_str(digits[0], int_str)
        return int_str, None
    if int_cnt == 1 and digits[0] in "+-":
        int_str = "0"
        if len(digits) > 1:
            int_str = round_int_str(digits[1], int_str)
        if int_str[0] == "1":
            int_str = digits[:1] + int_str
        return int_str, None
    if int_cnt <= len(digits):
        int_str = digits[:int_cnt]
        if int_cnt < len(digits):
            int_str = round_int_str(digits[int_cnt], int_str)
    else:
        int_str = digits + "0" * (int_cnt - len(digits))
    return int_str, None


def get_valid_float_prefix(sc, s):
    """getValidFloatPrefix (convert.go:430-478) -> (valid, err); str_ctx without EMPTY_NOT_ZERO = InSelectStmt or InDeleteStmt."""
    if not (sc.flags & EMPTY_NOT_ZERO) and s == "":
        return "0", None
    saw_dot = saw_digit = False
    valid_len = e_idx = 0
    for i, c in enumerate(s):
        if c in "+-":
            if i != 0 and i != e_idx + 1:  # "1e+1" is valid (and, as e_idx starts at 0, so is a sign at position 1)
                break
        elif c == ".":
            if saw_dot or e_idx > 0:
                break
            saw_dot = True
            if saw_digit:
                valid_len = i + 1
        elif c in "eE":
            if not saw_digit:
                break
            if e_idx != 0:
                break
            e_idx = i
        elif not _is_digit(c):
            break
        else:
            saw_digit = True
            valid_len = i + 1
    valid = s[:valid_len] or "0"
    err = None
    if valid_len == 0 or valid_len != len(s):
        err = _handle_truncate_error(sc)
    return valid, err


def get_valid_int_prefix(sc, s):
    """getValidIntPrefix (convert.go:249-282) -> (valid, err)."""
    if sc.flags & NOT_STRICT:
        float_prefix, err = get_valid_float_prefix(sc, s)
        if err:
            return float_prefix, err
        return float_str_to_int_str(sc, float_prefix)
    valid_len = 0
    for i, c in enumerate(s):
        if c in "+-" and i == 0:
            continue
        if _is_digit(c):
            valid_len = i + 1
            continue
        break
    valid = s[:valid_len] or "0"
    if valid_len == 0 or valid_len != len(s):
        return valid, _handle_truncate_error(sc)
    return valid, None


def str_to_int(b, str_ctx=CTX_SELECT):
    """StrToInt (convert.go:223-232) on the bytes of a cell -> (value, TSQ_S2I_* flags)."""
    sc = _Ctx(str_ctx)
    # Go strings are bytes: latin-1 maps every byte to one character and back
    s = trim_space(bytes(b)).decode("latin-1")
    try:
        valid, err = get_valid_int_prefix(sc, s)
    except IndexError:  # roundIntStr on a lone sign: the reference panics; the filter reports ErrOverflow with value 0
        return 0, sc.warn | ERR_OVF
    v, err1 = parse_int(valid)
    if err1:
        return v, sc.warn | ERR_OVF
    return v, sc.warn | (ERR_TRUNC if err == ERR_TRUNC else 0)
