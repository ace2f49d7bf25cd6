# TEST INFRASTRUCTURE ONLY: libmpcqp_emu_all.so = the objects of libmpcqp_emu_c2d.so (c2d.mk) + the InternalModel launcher
# (emu_im.cpp) + the second pass of the steady-state Riccati solve (emu_kf_dare_psd.cpp): every launcher that csrc/*_launch.h
# declares weak is present, so no entry point answers MPCQP_ERR_UNSUPPORTED for want of one.  A makefile of its own: the other
# libraries stay WITHOUT the launchers they are meant to lack.
include Makefile
libmpcqp_emu_all.so: $(STOCK_OBJS) $(EST_OBJS) emu_explicit.o emu_sim.o emu_est_init.o emu_kf_place.o emu_c2d.o emu_im.o emu_kf_dare_psd.o
-include emu_explicit.d emu_sim.d emu_est_init.d emu_kf_place.d emu_c2d.d emu_im.d emu_kf_dare_psd.d
