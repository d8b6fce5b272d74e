"""Programs for the plain layout's machine over the 64-bit field (sandstorm_amd/layouts/plain.py run): TEST INFRASTRUCTURE for
tests/test_gpu_gl64_device_trace.py.  busy_program() reaches every op1 source (imm, ap, fp, [op0]), every res logic, every pc update
(regular, abs, rel, jnz taken and not taken), every ap update (none, += res, += 1, += 2 by call), call / ret / assert_eq / nop,
products and sums that wrap p with operands p - 1 and >= 2^63, a jnz on such operands, 40 memory holes and a range-check span with
24 unused values, in more than 200 cycles before it idles in `jmp rel 0`."""
from sandstorm_amd import binary as bn
from sandstorm_amd.layouts import plain as pl

P = pl.P
ins = pl.instruction
F = bn
AE, AP1 = F.OPCODE_ASSERT_EQ, F.AP_ADD1


def push(value, off_op0=-1):
    """[ap] = value; ap++ (op0 = [fp + off_op0] is read and ignored)"""
    return [ins(0, off_op0, 1, (F.OP0_REG, F.OP1_IMM, AE, AP1)), value % P]


NOP = ins(-1, -1, -1, (F.DST_REG, F.OP0_REG, F.OP1_FP))                     # no opcode, pc + 1, ap as it is
IDLE = [ins(-1, -1, 1, (F.DST_REG, F.OP0_REG, F.OP1_IMM, F.PC_JUMP_REL)), 0]  # jmp rel 0


def jnz(off_dst, dst_fp=False):
    """jmp rel 2 if dst != 0 - taken or not, the next instruction"""
    return [ins(off_dst, -1, 1, ((F.DST_REG,) if dst_fp else ()) + (F.OP0_REG, F.OP1_IMM, F.PC_JNZ)), 2]


def busy_program(loops=50, program_base=1):
    prog = []
    prog += push(P - 1) + push(2**63) + push(2**63 + 12345) + push(3)             # fp + 0 .. fp + 3
    prog += [ins(0, -4, -3, (F.OP1_AP, F.RES_ADD, AE, AP1))]                      # fp + 4 = (p - 1) + 2^63: wraps
    prog += [ins(0, -5, -3, (F.OP1_AP, F.RES_MUL, AE, AP1))]                      # fp + 5 = (p - 1) (2^63 + 12345)
    prog += [ins(0, -5, -4, (F.OP1_AP, F.RES_MUL, AE, AP1))]                      # fp + 6 = 2^63 (2^63 + 12345)
    prog += [ins(0, -1, 1, (F.OP0_REG, F.OP1_FP, AE, AP1))]                       # fp + 7 = [fp + 1]: op1 from fp
    prog += [ins(0, -2, 2, (F.OP0_REG, AE, AP1))]                                 # fp + 8 = [[fp - 2] + 2] = [fp + 2]: op1 from [op0]
    prog += [ins(0, 0, 2, (F.OP0_REG, F.OP1_FP, F.RES_MUL, AE, AP1))]             # fp + 9 = [fp] [fp + 2]
    prog += jnz(-2)                                                              # dst = 2^63 + 12345: taken
    prog += jnz(0, dst_fp=True)                                                  # dst = p - 1: taken
    prog += push(0)                                                              # fp + 10
    prog += jnz(-1)                                                              # dst = 0: not taken
    prog += [NOP]
    prog += [ins(-1, -1, 1, (F.DST_REG, F.OP0_REG, F.OP1_IMM, F.AP_ADD)), 40]     # ap += 40: fp + 11 .. fp + 50 stay untouched
    prog += push(5, off_op0=-30)                                                 # reads a program word 30 below fp: the range-check span
    prog += [ins(-1, -1, 1, (F.DST_REG, F.OP0_REG, F.OP1_IMM, F.PC_JUMP_ABS)), program_base + len(prog) + 2]      # jmp abs: the next instruction
    prog += push(3) + push(loops)                                                # x, counter
    loop = ([ins(0, -2, -2, (F.OP1_AP, F.RES_MUL, AE, AP1))]                      # [ap] = [ap - 2]^2
            + [ins(0, -1, 1, (F.OP1_IMM, F.RES_ADD, AE, AP1)), 7]                 # [ap] = [ap - 1] + 7
            + [ins(0, -3, 1, (F.OP1_IMM, F.RES_ADD, AE, AP1)), P - 1])            # [ap] = [ap - 3] - 1
    prog += loop
    prog += [ins(-1, -1, 1, (F.OP0_REG, F.OP1_IMM, F.PC_JNZ)), (P - len(loop)) % P]
    prog += [ins(0, 1, 1, (F.OP1_IMM, F.PC_JUMP_REL, F.OPCODE_CALL)), 4]          # call rel 4
    prog += IDLE
    prog += [ins(0, -4, -3, (F.OP0_REG, F.OP1_FP, F.RES_MUL, AE, AP1))]           # f: [ap] = [fp - 4] [fp - 3]
    prog += [ins(-2, -1, -1, (F.DST_REG, F.OP0_REG, F.OP1_FP, F.PC_JUMP_ABS, F.OPCODE_RET))]
    return prog


def busy_cycles(loops=50):
    """the cycles busy_program runs before it idles"""
    prog = busy_program(loops)
    states, _ = pl.run(prog, 1024)
    idle = states[-1].pc
    return next(k for k, s in enumerate(states) if s.pc == idle)


def wide_offsets_program():
    """a 16-cycle run whose range-check pool spans more unused values than the trace has cycles (one operand read 20 below fp, out of
    the program), with no memory hole beyond the two cells of main's frame: 24 program words, all public"""
    prog = push(3, off_op0=-20) + IDLE
    return prog + [0] * (24 - len(prog))


def long_program(words=40):
    """more public memory than a 16-cycle trace has cells for"""
    prog = push(3) + IDLE
    return prog + [0] * (words - len(prog))


def holes_program():
    """ap += 40, then a write: more memory holes than a 16-cycle trace has gap cells"""
    return push(3) + [ins(-1, -1, 1, (F.DST_REG, F.OP0_REG, F.OP1_IMM, F.AP_ADD)), 40] + push(4) + IDLE
