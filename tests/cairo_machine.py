"""A minimal Cairo machine over the 252-bit prime and one synthetic program for it (test infrastructure).

The committed golden runs idle in `jmp rel 0` for all but a few hundred cycles, and what they compute stays small.  `synthetic_run`
makes a run whose first ~1 900 cycles - fourteen 128-cycle workgroups of the device's CPU kernel and more - are busy with 252-bit arithmetic:
assert_eq with add and with mul on operands near p (as immediates), a counted `jnz` loop whose tested value climbs from 2^249 past
2^250 to the last step below p and from there to zero, `call` / `ret`, `jmp abs`, `ap += res` over a stretch of memory nothing touches (the gap
fillers' work), an operand read through `[op0]`, and the final `jmp rel 0`.

The machine is the state transition of the Cairo paper (section 4.5) as sandstorm_amd/layouts/plain.py::run has it for the 64-bit
field, with the memory filled in as assert_eq / call write it.  The statements are laid out like sandstorm_amd/examples.py's: every
builtin segment of the layout, sized for the step count, back to back behind the execution segment, nothing of them used."""
from sandstorm_amd import binary as bn
from sandstorm_amd.layouts.plain import instruction
from sandstorm_amd.public_input import AirPublicInput

P = bn.P
LOOPS = 460                                   # 4 cycles each
GAP = 40                                      # addresses `ap += GAP` leaves untouched


def _res(w, pc, ap, fp, memory):
    if w.pc_update == 4:
        d = memory[w.dst_addr(ap, fp)] % P
        return pow(d, -1, P) if d else 0
    op0, op1 = memory[w.op0_addr(ap, fp)], memory[w.op1_addr(pc, ap, fp, memory)]
    return op1 % P if w.res_logic == 0 else (op0 + op1) % P if w.res_logic == 1 else op0 * op1 % P


def run(program, n_steps, program_base=1):
    """program = instruction words and immediates, expected to end in `jmp rel 0`; runs n_steps steps.
    -> (register states, memory list indexed by address, None = never accessed)"""
    execution_base = program_base + len(program)
    memory = [None] * program_base + [w % P for w in program] + [None] * (8 * LOOPS + 4 * GAP + 256)
    # main's frame starts behind the two cells of its caller's (saved fp, return pc).  Nothing is stored there: main never returns, so no
    # instruction reads the saved fp, which stays None - one more gap address - and the return pc is a cell only as far as an instruction
    # names [fp - 1] as an operand it ignores, which reads it as 0 like any other such cell.
    ap, fp, pc = execution_base + 2, execution_base + 2, program_base
    states = []
    for _ in range(n_steps):
        states.append(bn.RegisterState(ap, fp, pc))
        w = bn.Word(memory[pc])
        size = 1 + w.flag(bn.OP1_IMM)
        dst_addr, op0_addr = w.dst_addr(ap, fp), w.op0_addr(ap, fp)
        if w.flag(bn.OPCODE_CALL):
            memory[dst_addr], memory[op0_addr] = fp, pc + size
        if memory[op0_addr] is None:
            memory[op0_addr] = 0                                                      # an operand the instruction ignores
        op1_addr = w.op1_addr(pc, ap, fp, memory)
        if memory[op1_addr] is None:
            memory[op1_addr] = 0
        if w.flag(bn.OPCODE_ASSERT_EQ) and memory[dst_addr] is None:
            memory[dst_addr] = _res(w, pc, ap, fp, memory)
        if memory[dst_addr] is None:
            memory[dst_addr] = 0
        dst = memory[dst_addr]
        res = _res(w, pc, ap, fp, memory)
        if w.flag(bn.OPCODE_ASSERT_EQ) and dst != res:
            raise ValueError("assert_eq fails at pc %d" % pc)
        if w.pc_update == 4:
            npc = pc + size if dst == 0 else (pc + memory[op1_addr]) % P
        else:
            npc = pc + size if w.pc_update == 0 else res if w.pc_update == 1 else (pc + res) % P
        nap = ap + (res if w.ap_update == 1 else w.ap_update // 2) + (2 if w.flag(bn.OPCODE_CALL) else 0)
        nfp = ap + 2 if w.flag(bn.OPCODE_CALL) else dst if w.flag(bn.OPCODE_RET) else fp
        ap, fp, pc = nap % P, nfp, npc
        if max(ap, fp, pc) >> 63:
            raise ValueError("a register left the addresses trace.bin can hold")
    top = max(a for a, v in enumerate(memory) if v is not None)
    return states, memory[:top + 1]


def synthetic_program(program_base=1):
    """-> the words.  The loop's counter c starts at p - LOOPS * s with s = (p - 2^249) // LOOPS and gains s per round: the values the
    `jnz` tests (and the device inverts) run from about 2^249 to p - s, then 0."""
    F = bn
    AE, AP1 = F.OPCODE_ASSERT_EQ, F.AP_ADD1
    step = (P - 2**249) // LOOPS
    start = P - LOOPS * step
    assert 2**249 <= start < 2**250 < 2**251 - 2 * step < start + (LOOPS - 1) * step < P
    push_imm = lambda v: [instruction(0, -1, 1, (F.OP0_REG, F.OP1_IMM, AE, AP1)), v % P]            # [ap] = v; ap++  (op0 = [fp - 1], ignored)
    prog = push_imm(P - 2) + push_imm(start)                                               # x, c
    loop = (
        [instruction(0, -2, -2, (F.OP1_AP, F.RES_MUL, AE, AP1))]                           # [ap] = [ap-2] * [ap-2]; ap++        x^2
        + [instruction(0, -1, 1, (F.OP1_IMM, F.RES_ADD, AE, AP1)), P - 3]                  # [ap] = [ap-1] + (p - 3); ap++       x' = x^2 - 3
        + [instruction(0, -3, 1, (F.OP1_IMM, F.RES_ADD, AE, AP1)), step]                   # [ap] = [ap-3] + s; ap++             c' = c + s
    )
    prog += loop
    prog += [instruction(-1, -1, 1, (F.OP0_REG, F.OP1_IMM, F.PC_JNZ)), (P - len(loop)) % P]          # jmp rel -len(loop) if [ap-1] != 0
    # [ap-2] = the last x, [ap-1] = 0.  A pointer to the first x, then an operand through it: op1 = [[ap-1] + 0]
    tail_at = len(prog)
    tail = push_imm(0)                                                                      # the pointer (patched: it depends on the length)
    tail += [instruction(0, -1, 0, (AE, AP1))]                                             # [ap] = [[ap-1] + 0]; ap++           = p - 2
    tail += [instruction(0, -1, -4, (F.OP1_AP, F.RES_MUL, AE, AP1))]                       # [ap] = [ap-1] * [ap-4]; ap++        (p - 2) * last x
    tail += [instruction(0, 1, 1, (F.OP1_IMM, F.PC_JUMP_REL, F.OPCODE_CALL)), 0]           # call f (rel, patched)
    call_at = tail_at + len(tail) - 2
    tail += [instruction(-1, -1, 1, (F.DST_REG, F.OP0_REG, F.OP1_IMM, F.PC_JUMP_ABS)), 0]  # jmp abs over the dead word (patched)
    jmp_at = tail_at + len(tail) - 2
    tail += [instruction(0, -1, 1, (F.OP0_REG, F.OP1_IMM, AE, AP1))]                       # dead: never run (its immediate is the next word)
    landing = tail_at + len(tail)
    tail += [instruction(-1, -1, 1, (F.DST_REG, F.OP0_REG, F.OP1_IMM, F.AP_ADD)), GAP]     # ap += GAP: the cells in between stay untouched
    tail += push_imm(P - 1)                                                                 # the first cell behind the gap
    tail += [instruction(0, -1, -1, (F.OP1_AP, F.RES_MUL, AE, AP1))]                       # [ap] = [ap-1] * [ap-1]; ap++        (p - 1)^2 = 1
    tail += [instruction(-1, -1, 1, (F.OP0_REG, F.OP1_IMM, F.PC_JNZ)), 2]                  # jnz over nothing, taken: dst = 1
    tail += push_imm(0)
    tail += [instruction(-1, -1, 1, (F.OP0_REG, F.OP1_IMM, F.PC_JNZ)), 77]                 # jnz not taken: dst = 0
    tail += [instruction(-1, -1, 1, (F.DST_REG, F.OP0_REG, F.OP1_IMM, F.PC_JUMP_REL)), 0]  # jmp rel 0
    f_at = tail_at + len(tail)
    tail += [instruction(0, -3, -4, (F.OP0_REG, F.OP1_FP, F.RES_MUL, AE, AP1))]            # f: [ap] = [fp-3] * [fp-4]; ap++
    tail += [instruction(0, -1, 1, (F.OP1_IMM, F.RES_ADD, AE, AP1)), 2**251]               # [ap] = [ap-1] + 2^251; ap++
    tail += [instruction(-2, -1, -1, (F.DST_REG, F.OP0_REG, F.OP1_FP, F.PC_JUMP_ABS, F.OPCODE_RET))]   # ret
    prog += tail
    prog[tail_at + 1] = program_base + len(prog) + 2                                        # the first x: the first cell of main's frame
    prog[call_at + 1] = f_at - call_at
    prog[jmp_at + 1] = program_base + landing
    return prog


def synthetic_run(layout, log_steps):
    """-> (register states, memory, AirPublicInput) of the synthetic program as a 2^log_steps-step statement of `layout`"""
    from sandstorm_amd.layouts import recursive as rec, starknet as sk
    n_steps = 1 << log_steps
    program = synthetic_program()
    states, memory = run(program, n_steps)
    last = states[-1]
    w = bn.Word(memory[last.pc])
    if not (w.pc_update == 2 and memory[last.pc + 1] == 0 and states[-2] == last):
        raise ValueError("the run does not end in `jmp rel 0`")
    offsets = [o for st in states for v in [bn.Word(memory[st.pc])] for o in (v.off_dst, v.off_op0, v.off_op1)]
    addr = last.ap
    seg = {name: None for name in ("program", "execution", "output", "pedersen", "range_check", "ecdsa", "bitwise", "ec_op", "poseidon")}
    seg["program"], seg["execution"], seg["output"] = (1, last.pc), (1 + len(program) + 2, last.ap), (addr, addr)
    if layout == "recursive":
        builtins = (("pedersen", rec.PEDERSEN_BUILTIN_RATIO, 3), ("range_check", rec.RANGE_CHECK_BUILTIN_RATIO, 1), ("bitwise", rec.BITWISE_RATIO, 5))
    else:
        builtins = (("pedersen", sk.PEDERSEN_BUILTIN_RATIO, 3), ("range_check", sk.RANGE_CHECK_BUILTIN_RATIO, 1), ("ecdsa", sk.ECDSA_BUILTIN_RATIO, 2),
                    ("bitwise", sk.BITWISE_RATIO, 5), ("ec_op", sk.EC_OP_BUILTIN_RATIO, 7), ("poseidon", sk.POSEIDON_RATIO, 6))
    for name, ratio, cells in builtins:
        seg[name] = (addr, addr)                     # begin = stop: the program uses nothing of the segment
        addr += cells * (n_steps // ratio)
    public_memory = [(1 + k, v % P) for k, v in enumerate(program)]
    return states, memory, AirPublicInput(layout, min(offsets), max(offsets), n_steps, seg, public_memory)


def busy_cycles(states):
    """cycles before the run settles in its final state"""
    return next(k for k, st in enumerate(states) if st == states[-1])
