// ctx_switch.h -- TEST-ONLY: ppg_emu_ctx_switch of wave_emu.h, the emulator's fiber switch.  Included by exactly ONE unit of a
// program or library (ppg_emu.cpp; san_main.h for the stand-alone sanitizer programs).
#pragma once

#if defined(__x86_64__)
__asm__(
    ".text\n"
    ".globl ppg_emu_ctx_switch\n"
    ".type ppg_emu_ctx_switch,@function\n"
    "ppg_emu_ctx_switch:\n"
    "  pushq %rbp\n  pushq %rbx\n  pushq %r12\n  pushq %r13\n  pushq %r14\n  pushq %r15\n"
    "  movq %rsp, (%rdi)\n"
    "  movq %rsi, %rsp\n"
    "  popq %r15\n  popq %r14\n  popq %r13\n  popq %r12\n  popq %rbx\n  popq %rbp\n"
    "  ret\n"
    ".size ppg_emu_ctx_switch, .-ppg_emu_ctx_switch\n");
#else
#error "wave emulator context switch is written for x86-64"
#endif
