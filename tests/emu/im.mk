# TEST INFRASTRUCTURE ONLY: libmpcqp_emu_im.so = libmpcqp_emu_sim.so + the InternalModel launcher (emu_im.cpp).  A makefile of
# its own: the other libraries stay WITHOUT that launcher.
include Makefile
libmpcqp_emu_im.so: $(STOCK_OBJS) $(EST_OBJS) emu_explicit.o emu_sim.o emu_im.o
-include emu_explicit.d emu_sim.d emu_im.d
